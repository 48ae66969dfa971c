"""
numpy checker for the noisy forward (qhea_model_forward_noisy, include/quanonet_hea.h):
  * philox4x32 -- Philox4x32-10, vectorised over counters;
  * stream, shot_values -- the random stream of a call's (row, trajectory) pairs and the tail of shot mode, shared with
    tests/device_traj_reference.py;
  * replay_values -- a gate-by-gate fp64 statevector replay of every (row, trajectory) that consumes the header's random
    stream: a trajectory's value (expectation mode: its exact read-out with readout error folded in; shot mode: one sampled,
    readout-flipped bitstring);
  * exact_values -- the same channels and readout confusion on a density matrix (n <= 5): the exact noisy expectation;
  * readout_diag -- diag' of the header (ham_diag under readout error).
Circuit conventions are oracle.hea_oracle's (little-endian wires, RX / RY / RZ, ring CNOT((i+1)%n -> i)).
"""
import numpy as np

from oracle import hea_oracle as O

WIDE = np.clongdouble                        # the extended-precision type of the trajectory references (x87: 64-bit mantissa)
M32 = np.uint64(0xFFFFFFFF)
_PM = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
_PW = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))
SQ = 1.0 / np.sqrt(2.0)


def philox4x32(ctr, key):
    """Philox4x32-10 of counters ctr = (c0, c1, c2, c3) (ints or equal-length arrays) under key = (k0, k1): four uint64 arrays
    of 32-bit words."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32 for v in ctr]
    c = np.broadcast_arrays(*c)
    c0, c1, c2, c3 = [v.copy() for v in c]
    k0, k1 = np.uint64(key[0]) & M32, np.uint64(key[1]) & M32
    for r in range(10):
        if r:
            k0 = (k0 + _PW[0]) & M32
            k1 = (k1 + _PW[1]) & M32
        p0 = _PM[0] * c0
        p1 = _PM[1] * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def threshold(p):
    """An event of probability p happens iff its word is < threshold(p) (p 2^32, exact in fp64, floored)."""
    return int(float(p) * 4294967296.0)


def n_locations(n, cfgs):
    return sum(n + 2 * n * ld for _, ld in cfgs)


def real_of(dtype):
    """the real scalar type of a complex dtype.  Every replay and walk of the trajectory references takes dtype=np.complex128 by
    default; with np.clongdouble the inputs stay the float64 data they are and everything computed from them -- half angles,
    sin / cos / exp, sqrt(1 - gamma), the read-out weights and every sum -- is done in the wide type.  Random words and the
    thresholds they are compared with stay integers."""
    return np.finfo(dtype).dtype.type


# ---- gates on psi[M, 2^n] (complex) --------------------------------------------------------------------------------------
def _rx(psi, n, q, theta, dagger=False):
    """oracle.hea_oracle._rx without its cast of the angle to float64 (the same bits for a float64 angle)"""
    th = np.asarray(theta)
    if th.ndim == 1:
        th = th[:, None]
    c = np.cos(th / 2)
    s = np.sin(th / 2)
    if dagger:
        s = -s
    O._apply_1q(psi, n, q, c, -1j * s, -1j * s, c)


def _pauli(psi, n, q, p, sel):
    """p in 1..3 (X, Y, Z) on wire q for the rows sel (boolean mask)."""
    if not np.any(sel):
        return
    i0, i1 = O._pairs(n, q)
    a0 = psi[np.ix_(sel, i0)]
    a1 = psi[np.ix_(sel, i1)]
    if p == 1:
        psi[np.ix_(sel, i0)], psi[np.ix_(sel, i1)] = a1, a0
    elif p == 2:
        psi[np.ix_(sel, i0)], psi[np.ix_(sel, i1)] = -1j * a1, 1j * a0
    else:
        psi[np.ix_(sel, i1)] = -a1


def _basis_change(psi, n, pauli):
    """H (X read-out) or H S^dagger (Y read-out) on every wire."""
    if pauli == 'Z':
        return
    sq = 1.0 / np.sqrt(real_of(psi.dtype)(2.0))
    for q in range(n):
        if pauli == 'Y':
            O._apply_1q(psi, n, q, 1.0, 0.0, 0.0, -1j)
        O._apply_1q(psi, n, q, sq, sq, sq, -sq)


def readout_diag(diag, n, q):
    """diag'[k] = sum_j prod_i (bit_i(j) != bit_i(k) ? q : 1 - q) diag[j], j in index order, i in wire order."""
    D = 1 << n
    out = np.zeros(D)
    for k in range(D):
        acc = 0.0
        for j in range(D):
            w = 1.0
            for i in range(n):
                w *= q if ((j ^ k) >> i) & 1 else 1.0 - q
            acc += w * diag[j]
        out[k] = acc
    return out


def _readout_weights(n, offset, coeff, ham_diag, q, real=np.float64):
    """(off_term, h[k]) of expectation mode: value = off_term + sum_k p_k h[k]."""
    k = np.arange(1 << n)
    if ham_diag is not None:
        assert real is np.float64, 'readout_diag is fp64: noisy_traj_grad_reference.readout_table takes a type'
        return 0.0, readout_diag(np.asarray(ham_diag, np.float64), n, q)
    pop = sum((k >> i) & 1 for i in range(n))
    if real is np.float64:
        return float(offset), coeff * (1.0 - 2.0 * q) * (n - 2.0 * pop)
    return real(offset), real(coeff) * (1 - 2 * real(q)) * (n - 2 * pop.astype(real))


def stream(B, T, row0, seed):
    """words(c) of a call's B * T values, row-major: the four word arrays of Philox call c for every (row, trajectory)."""
    ident = (int(B), int(T), int(row0), int(seed))
    if ident in _STREAMS:
        return _STREAMS[ident]
    rows = np.repeat(np.arange(B, dtype=np.uint64) + np.uint64(row0), T)
    trajs = np.tile(np.arange(T, dtype=np.uint64), B)
    key = (int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    cache = {}

    def words(c):
        if c not in cache:
            cache[c] = philox4x32((np.uint64(c), trajs, rows & M32, rows >> np.uint64(32)), key)
            for a in cache[c]:
                a.setflags(write=False)
        return cache[c]

    if B * T <= 64:                          # a shift rule replays the same few rows once per angle: keep their words
        if len(_STREAMS) >= 8:
            _STREAMS.pop(next(iter(_STREAMS)))
        _STREAMS[ident] = words
    return words


_STREAMS = {}


def shot_values(prob, words, call0, n, thr, offset, coeff, ham_diag):
    """Shot mode's tail.  u (53 bits of call0's first two words) picks the first k with u < cdf[k] (prob as given, index order,
    fp64), or the last k of positive weight; bit i of it flips iff word 2 + i of the calls from call0 on is below thr(i, the
    bit's true value); the value of the string that is read."""
    wm = words(call0)
    u = ((wm[0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (wm[1] >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    hit = u[:, None] < np.cumsum(prob, axis=1)
    last = (1 << n) - 1 - np.argmax((prob > 0)[:, ::-1], axis=1)
    true = np.where(hit.any(axis=1), np.argmax(hit, axis=1), last)
    out = true.copy()
    for i in range(n):
        m = 2 + i
        flip = words(call0 + m // 4)[m % 4] < thr(i, (true >> i) & 1)
        out = out ^ (flip.astype(np.int64) << i)
    if ham_diag is not None:
        return np.asarray(ham_diag, np.float64)[out]
    pop = sum((out >> i) & 1 for i in range(n))
    return offset + coeff * (n - 2.0 * pop)


def replay_values(n, cfgs, x, w, noise, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', row0=0, dtype=np.complex128,
                  weights=None):
    """
    values[B, T]: trajectory t of row b (global row row0 + b) replayed gate by gate on the header's random stream (no bias).
    noise: an object with p1, p2, readout, shots, trajectories, seed (quanonet_amd.noise.NoiseModel or alike).
    dtype: real_of.  weights: (off_term, h'[k]) of expectation mode where the caller has them (a wide diagonal read-out).
    """
    real = real_of(dtype)
    x = np.asarray(x, real)
    w = np.asarray(w, real)
    B = x.shape[0]
    T = int(noise.shots) if noise.shots > 0 else int(noise.trajectories)
    words = stream(B, T, row0, noise.seed)

    def draw(loc, p, two):
        wd = words(loc // 2)
        w0, w1 = wd[2 * (loc % 2)], wd[2 * (loc % 2) + 1]
        err = w0 < np.uint64(threshold(p))
        idx = (w1 * np.uint64(15 if two else 3)) >> np.uint64(32)
        return err, idx.astype(np.int64)

    X = np.repeat(x, T, axis=0)
    M = B * T
    psi = np.zeros((M, 1 << n), dtype=dtype)
    psi[:, 0] = 1.0
    loc, col, s = 0, 0, 0
    for n_enc, ld in cfgs:
        assert n_enc == n
        for q in range(n):
            _rx(psi, n, q, X[:, col + q])
            err, idx = draw(loc + q, noise.p1, False)
            for p in (1, 2, 3):
                _pauli(psi, n, q, p, err & (idx == p - 1))
        col += n
        loc += n
        for _ in range(ld):
            for q in range(n):
                O._ry(psi, n, q, w[s, 0, q])
                O._rz(psi, n, q, w[s, 1, q])
                O._ry(psi, n, q, w[s, 2, q])
                err, idx = draw(loc + q, noise.p1, False)
                for p in (1, 2, 3):
                    _pauli(psi, n, q, p, err & (idx == p - 1))
            for j in range(n):
                c, t = (j + 1) % n, j
                O._cnot(psi, n, c, t)
                err, idx = draw(loc + n + j, noise.p2, True)
                code = idx + 1
                for p in (1, 2, 3):
                    _pauli(psi, n, c, p, err & ((code >> 2) == p))
                    _pauli(psi, n, t, p, err & ((code & 3) == p))
            loc += 2 * n
            s += 1
    assert loc == n_locations(n, cfgs)
    pauli = O._check_pauli(ham_pauli, ham_diag)
    _basis_change(psi, n, pauli)
    prob = psi.real ** 2 + psi.imag ** 2
    if noise.shots == 0:
        off, h = weights if weights is not None else _readout_weights(n, offset, coeff, ham_diag, float(noise.readout), real)
        vals = off + prob @ h
    else:
        thr = np.uint64(threshold(noise.readout))
        vals = shot_values(prob, words, (loc + 1) // 2, n, lambda i, bit: thr, offset, coeff, ham_diag)    # prob as it is
    return vals.reshape(B, T)


# ---- density matrix rho[B, D, D] -------------------------------------------------------------------------------------------
def _mat(rho, n, q, m):
    """rho <- M_q rho M_q^dagger, m = (m00, m01, m10, m11), each a scalar or a (B,) array."""
    m = [np.asarray(v, np.complex128).reshape(-1, 1, 1) if np.ndim(v) else v for v in m]
    i0, i1 = O._pairs(n, q)
    a0, a1 = rho[:, i0, :].copy(), rho[:, i1, :].copy()
    rho[:, i0, :] = m[0] * a0 + m[1] * a1
    rho[:, i1, :] = m[2] * a0 + m[3] * a1
    b0, b1 = rho[:, :, i0].copy(), rho[:, :, i1].copy()
    rho[:, :, i0] = b0 * np.conj(m[0]) + b1 * np.conj(m[1])
    rho[:, :, i1] = b0 * np.conj(m[2]) + b1 * np.conj(m[3])


_PAULI_M = {1: (0, 1, 1, 0), 2: (0, -1j, 1j, 0), 3: (1, 0, 0, -1)}


def _depolarize(rho, n, wires, p):
    """(1 - p) rho + p / (4^k - 1) sum over non-identity Pauli strings P on `wires` of P rho P."""
    if p == 0.0:
        return rho
    k = len(wires)
    acc = (1.0 - p) * rho
    for code in range(1, 4 ** k):
        r = rho.copy()
        for i, wire in enumerate(wires):
            pc = (code >> (2 * (k - 1 - i))) & 3
            if pc:
                _mat(r, n, wire, _PAULI_M[pc])
        acc = acc + p / (4 ** k - 1) * r
    return acc


def exact_values(n, cfgs, x, w, p1, p2, readout, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z'):
    """The exact noisy expectation per row (no bias): density-matrix evolution through the same channels, then the readout
    confusion (n <= 5).  Also returns the per-row variance of one shot's value (second moment minus the square)."""
    assert n <= 5
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, D = x.shape[0], 1 << n
    rho = np.zeros((B, D, D), dtype=np.complex128)
    rho[:, 0, 0] = 1.0
    col, s = 0, 0
    for n_enc, ld in cfgs:
        for q in range(n):
            c, sn = np.cos(x[:, col + q] / 2), np.sin(x[:, col + q] / 2)
            _mat(rho, n, q, (c, -1j * sn, -1j * sn, c))
            rho = _depolarize(rho, n, [q], p1)
        col += n
        for _ in range(ld):
            for q in range(n):
                for ang, kind in ((w[s, 0, q], 'y'), (w[s, 1, q], 'z'), (w[s, 2, q], 'y')):
                    c, sn = np.cos(ang / 2), np.sin(ang / 2)
                    if kind == 'y':
                        _mat(rho, n, q, (c, -sn, sn, c))
                    else:
                        _mat(rho, n, q, (np.exp(-0.5j * ang), 0, 0, np.exp(0.5j * ang)))
                rho = _depolarize(rho, n, [q], p1)
            for j in range(n):
                ctl, t = (j + 1) % n, j
                kk = np.arange(D)
                src = np.where((kk >> ctl) & 1, kk ^ (1 << t), kk)
                rho = rho[:, src][:, :, src]
                rho = _depolarize(rho, n, [ctl, t], p2)
            s += 1
    pauli = O._check_pauli(ham_pauli, ham_diag)
    if pauli != 'Z':
        for q in range(n):
            if pauli == 'Y':
                _mat(rho, n, q, (1.0, 0.0, 0.0, -1j))
            _mat(rho, n, q, (SQ, SQ, SQ, -SQ))
    prob = np.real(np.einsum('bkk->bk', rho))
    # readout confusion: read j given true k with prod_i (bits differ ? q : 1 - q)
    kk = np.arange(D)
    conf = np.ones((D, D))
    for i in range(n):
        diff = ((kk[:, None] ^ kk[None, :]) >> i) & 1
        conf *= np.where(diff, readout, 1.0 - readout)
    pread = prob @ conf                                  # [B, D] over read bitstrings
    if ham_diag is not None:
        hv = np.asarray(ham_diag, np.float64)
    else:
        pop = sum((kk >> i) & 1 for i in range(n))
        hv = offset + coeff * (n - 2.0 * pop)
    mean = pread @ hv
    var = pread @ (hv * hv) - mean ** 2
    return mean, var
