"""
numpy checker for the quantum-jump trajectories under the device noise model (qhea_model_forward_noisy_device,
include/quanonet_hea.h):
  * jump_pairs -- (gamma, pz) of every site at its folded duration, from the header's formulas;
  * site_kraus / site_channel -- the three Kraus operators of a (gamma, pz) pair and the channel they make on a 2 x 2 matrix;
  * readout_weights -- h(k) / diag' of expectation mode under the asymmetric readout;
  * replay_values -- a gate-by-gate fp64 statevector replay of every (row, trajectory) on the header's random stream, the state
    normalised at every damping event exactly as the header words it.  It also counts the events that fired.
Circuit conventions are oracle.hea_oracle's; gates, the stream, thresholds and shot mode's tail are tests/noise_oracle.py's.
"""
import numpy as np

from oracle import hea_oracle as O
from tests import noise_oracle as NO

ENC, ROT, CTL, TGT = 0, 1, 2, 3


def site_duration(n, nz, site, q):
    idle = bool(nz['idle'])
    if site == ENC:
        return nz['t_rx']
    if site == ROT:
        return nz['t_rot'] + ((q - 1) * nz['t_cx'] if idle and q >= 1 else 0.0)
    if site == CTL:
        return nz['t_cx']
    return ((n - 1 if q == 0 else n - q) if idle else 1) * nz['t_cx']


def jump_pair(tau, T1, T2, real=np.float64):
    if real is not np.float64:
        tau, T1, T2 = real(tau), real(T1), real(T2)
    gamma = 1.0 - np.exp(-tau / T1) if np.isfinite(T1) else 0.0
    total = np.exp(-tau / T2) if np.isfinite(T2) else 1.0
    f = min(total / np.sqrt(1.0 - gamma), 1.0) if gamma < 1.0 else 0.0
    return gamma, (1.0 - f) / 2.0


def jump_pairs(n, nz, real=np.float64):
    """[4, n, 2]: (gamma, pz) per site and wire, in `real` from the float64 durations and times"""
    out = np.zeros((4, n, 2), dtype=real)
    for site in range(4):
        for q in range(n):
            out[site, q] = jump_pair(site_duration(n, nz, site, q), nz['t1'][q], nz['t2'][q], real)
    return out


def site_kraus(gamma, pz):
    """dephasing (Z with probability pz) after damping: the operators Z^b K for K in (no jump, jump) with their weights"""
    k0 = np.array([[1, 0], [0, np.sqrt(1.0 - gamma)]], dtype=np.complex128)
    k1 = np.array([[0, np.sqrt(gamma)], [0, 0]], dtype=np.complex128)
    z = np.diag([1.0, -1.0]).astype(np.complex128)
    return [(1.0 - pz, k0), (1.0 - pz, k1), (pz, z @ k0), (pz, z @ k1)]


def site_channel(rho2, gamma, pz):
    """Z-dephasing commutes with damping as a channel, so the order of the two events does not show here"""
    return sum(wt * K @ rho2 @ K.conj().T for wt, K in site_kraus(gamma, pz))


def readout_weights(n, offset, coeff, ham_diag, r01, r10, real=np.float64):
    """(off_term, h[k]): value = off_term + sum_k p_k h[k], k the true string"""
    D = 1 << n
    kk = np.arange(D)
    if real is not np.float64:
        r01, r10 = np.asarray(r01, np.float64).astype(real), np.asarray(r10, np.float64).astype(real)
        offset, coeff = real(offset), real(coeff)
    if ham_diag is None:
        h = np.zeros(D, dtype=real)
        for i in range(n):
            h += np.where((kk >> i) & 1, -(1.0 - 2.0 * r10[i]), 1.0 - 2.0 * r01[i])
        return offset if real is not np.float64 else float(offset), coeff * h
    h = np.asarray(ham_diag, np.float64).astype(real)
    for i in range(n):
        e = np.where((kk >> i) & 1, r10[i], r01[i])
        h = (1.0 - e) * h + e * h[kk ^ (1 << i)]
    return 0.0, h


def n_calls(n, cfgs):
    return sum(n + 3 * n * ld for _, ld in cfgs)


def replay_values(n, cfgs, x, w, nz, shots, trajectories, seed, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', row0=0,
                  counts=None, dtype=np.complex128):
    """
    values[B, T]: trajectory t of row b (global row row0 + b), no bias.  nz: the dict of tests/device_noise_reference.py.
    counts (a dict, optional) receives the number of Paulis, dephasings and jumps that fired.  dtype: noise_oracle.real_of
    (expectation mode; the dephasing thresholds are taken from the float64 pz in either type).
    """
    real = NO.real_of(dtype)
    assert real is np.float64 or shots == 0
    x = np.asarray(x, real)
    w = np.asarray(w, real)
    B = x.shape[0]
    T = int(shots) if shots > 0 else int(trajectories)
    words = NO.stream(B, T, row0, seed)
    jp = jump_pairs(n, nz, real)
    pz64 = jump_pairs(n, nz)[..., 1]
    fired = {'pauli': 0, 'dephasing': 0, 'jump': 0}

    M = B * T
    psi = np.zeros((M, 1 << n), dtype=dtype)
    psi[:, 0] = 1.0

    def pauli1(q, wd, p):
        err = wd[0] < np.uint64(NO.threshold(p))
        idx = ((wd[1] * np.uint64(3)) >> np.uint64(32)).astype(np.int64)
        fired['pauli'] += int(err.sum())
        for c in (1, 2, 3):
            NO._pauli(psi, n, q, c, err & (idx == c - 1))

    def relax(q, site, wd):
        gamma = jp[site, q, 0]
        zsel = wd[2] < np.uint64(NO.threshold(pz64[site, q]))
        fired['dephasing'] += int(zsel.sum())
        NO._pauli(psi, n, q, 3, zsel)
        if gamma == 0.0:
            return
        i0, i1 = O._pairs(n, q)
        a0, a1 = psi[:, i0], psi[:, i1]
        norm = np.sum(psi.real ** 2 + psi.imag ** 2, axis=1)
        P1 = np.sum(a1.real ** 2 + a1.imag ** 2, axis=1) / norm
        u = ((wd[3].astype(np.float64) + 0.5) * 2.0 ** -32).astype(real)
        fire = u < gamma * P1
        fired['jump'] += int(fire.sum())
        with np.errstate(divide='ignore', invalid='ignore'):
            jn = 1.0 / np.sqrt(P1 * norm)
            kn = 1.0 / np.sqrt((1.0 - gamma * P1) * norm)
        f = fire[:, None]
        psi[:, i0] = np.where(f, a1 * np.where(fire, jn, 0.0)[:, None], a0 * np.where(fire, 0.0, kn)[:, None])
        psi[:, i1] = np.where(f, 0.0, a1 * (np.sqrt(1.0 - gamma) * np.where(fire, 0.0, kn))[:, None])

    X = np.repeat(x, T, axis=0)
    call, col, s = 0, 0, 0
    for n_enc, ld in cfgs:
        assert n_enc == n
        for q in range(n):
            NO._rx(psi, n, q, X[:, col + q])
            wd = words(call + q)
            pauli1(q, wd, nz['p1'][q])
            relax(q, ENC, wd)
        col += n
        call += n
        for _ in range(ld):
            for q in range(n):
                O._ry(psi, n, q, w[s, 0, q])
                O._rz(psi, n, q, w[s, 1, q])
                O._ry(psi, n, q, w[s, 2, q])
                wd = words(call + q)
                pauli1(q, wd, nz['p1'][q])
                relax(q, ROT, wd)
            call += n
            for j in range(n):
                c, t = (j + 1) % n, j
                O._cnot(psi, n, c, t)
                wd = words(call + 2 * j)
                err = wd[0] < np.uint64(NO.threshold(nz['p2'][j]))
                code = ((wd[1] * np.uint64(15)) >> np.uint64(32)).astype(np.int64) + 1
                fired['pauli'] += int(err.sum())
                for p in (1, 2, 3):
                    NO._pauli(psi, n, c, p, err & ((code >> 2) == p))
                    NO._pauli(psi, n, t, p, err & ((code & 3) == p))
                relax(t, TGT, wd)
                relax(c, CTL, words(call + 2 * j + 1))
            call += 2 * n
            s += 1
    assert call == n_calls(n, cfgs)
    if counts is not None:
        counts.update(fired)
    pauli = O._check_pauli(ham_pauli, ham_diag)
    NO._basis_change(psi, n, pauli)
    prob = psi.real ** 2 + psi.imag ** 2
    prob = prob / prob.sum(axis=1, keepdims=True)
    r01, r10 = nz['readout01'], nz['readout10']
    if shots == 0:
        off, h = readout_weights(n, offset, coeff, ham_diag, r01, r10, real)
        vals = off + prob @ h
    else:
        thr = [(np.uint64(NO.threshold(r01[i])), np.uint64(NO.threshold(r10[i]))) for i in range(n)]
        vals = NO.shot_values(prob, words, call, n, lambda i, bit: np.where(bit == 1, thr[i][1], thr[i][0]), offset, coeff,
                              ham_diag)
    return vals.reshape(B, T)


def mean_and_stderr(vals):
    """what the finishing kernel reports for values[B, T] (no bias): mean, sample deviation / sqrt(T)"""
    T = vals.shape[1]
    mean = vals.mean(axis=1)
    if T == 1:
        return mean, np.zeros_like(mean)
    return mean, vals.std(axis=1, ddof=1) / np.sqrt(T)
