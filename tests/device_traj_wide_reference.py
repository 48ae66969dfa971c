"""
numpy restatement of the formulation of the workgroup-resident device-noise trajectory kernel
(qhea_model_forward_noisy_device_wide, quanonet_amd/csrc/hea_noise_device_wide.hip), generic in n >= 3:
  * the state of a sub-layer stays in the labels it had BEFORE the CNOT ring; the ring is one index map at the segment's end;
  * a Pauli frame (X mask, Z mask) per trajectory that the sampled Paulis, the dephasings AND the jumps update between the sites,
    pushed through every CNOT (x_t ^= x_c, z_c ^= z_t) and applied with the ring at the segment's end;
  * a damping site on wire w is diagonal on the stored amplitudes: "wire w reads |1>" is parity(k & mask) ^ bit w of the X mask,
    mask = site_mask(...) below (at most three stored bits);
  * the state is unnormalised with its squared norm N2 beside it: the jump fires iff u N2 < gamma M, a jump zeroes the
    amplitudes that read |0>, sets N2 = M and toggles bit w of the X mask (|0><1| = X . Pi_1); no jump scales the |1> half by
    sqrt(1 - gamma) and leaves N2 - gamma M; a power-of-two rescale behind a segment.
It runs on the header's Philox stream; tests/test_device_traj_wide_abi.py checks it against the literal gate-by-gate replay of
tests/device_traj_reference.py (values, and the number of Paulis, dephasings and jumps that fired).  The sums here are numpy's:
the kernel's summation orders are not restated, only its algebra.
"""
import numpy as np

from oracle import hea_oracle as O
from tests import noise_oracle as NO
from tests.device_traj_reference import CTL, ENC, ROT, TGT, jump_pairs, n_calls, readout_weights


def site_mask(n, kind, j):
    """(wire, stored-bit mask) of a site.  kind ENC / ROT: the site of wire j.  kind TGT / CTL: the site behind CNOT slot j,
    the state still stored in pre-ring labels."""
    if kind in (ENC, ROT):
        return j, 1 << j
    if kind == TGT:
        return (j, (1 << j) | (1 << (j + 1))) if j < n - 1 else (n - 1, (1 << (n - 1)) | 3)
    return (j + 1, 1 << (j + 1)) if j < n - 1 else (0, 3)


def ring_map(n):
    k = np.arange(1 << n)
    for i in range(n):
        k = k ^ (((k >> ((i + 1) % n)) & 1) << i)
    return k


def _parity(v):
    v = np.asarray(v, np.int64).copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> s
    return v & 1


def formulation_values(n, cfgs, x, w, nz, shots, trajectories, seed, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', row0=0,
                       counts=None):
    """values[B, T] as tests.device_traj_reference.replay_values returns them, computed the kernel's way"""
    assert n >= 3
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B = x.shape[0]
    T = int(shots) if shots > 0 else int(trajectories)
    words = NO.stream(B, T, row0, seed)
    jp = jump_pairs(n, nz)
    fired = {'pauli': 0, 'dephasing': 0, 'jump': 0}
    M = B * T
    D = 1 << n
    kk = np.arange(D)
    rows = np.arange(M)[:, None]
    psi = np.zeros((M, D), dtype=np.complex128)
    psi[:, 0] = 1.0
    N2 = np.ones(M)
    fx = np.zeros(M, np.int64)                     # the frame, in the labels of the circuit point reached
    fz = np.zeros(M, np.int64)

    def pauli_bits(p, wire):
        """frame bits of Pauli code p (0 I, 1 X, 2 Y, 3 Z) arrays on `wire`"""
        return (((p == 1) | (p == 2)).astype(np.int64) << wire), ((p >= 2).astype(np.int64) << wire)

    def relax(kind, j, wd):
        nonlocal psi, N2, fx, fz
        wire, mask = site_mask(n, kind, j)
        gamma, pz = jp[kind, wire]
        zsel = wd[2] < np.uint64(NO.threshold(pz))
        fired['dephasing'] += int(zsel.sum())
        fz ^= zsel.astype(np.int64) << wire
        if gamma == 0.0:
            return
        one = (_parity(kk & mask)[None, :] ^ ((fx >> wire) & 1)[:, None]).astype(bool)
        p = psi.real ** 2 + psi.imag ** 2
        Msum = np.where(one, p, 0.0).sum(axis=1)
        u = (wd[3].astype(np.float64) + 0.5) * 2.0 ** -32
        fire = u * N2 < gamma * Msum
        fired['jump'] += int(fire.sum())
        f = fire[:, None]
        psi = np.where(f, np.where(one, psi, 0.0), np.where(one, psi * np.sqrt(1.0 - gamma), psi))
        N2 = np.where(fire, Msum, N2 - gamma * Msum)
        fx ^= fire.astype(np.int64) << wire

    def site1(kind, q, wd, p1):
        nonlocal fx, fz
        err = wd[0] < np.uint64(NO.threshold(p1))
        fired['pauli'] += int(err.sum())
        code = np.where(err, ((wd[1] * np.uint64(3)) >> np.uint64(32)).astype(np.int64) + 1, 0)
        bx, bz = pauli_bits(code, q)
        fx ^= bx
        fz ^= bz
        relax(kind, q, wd)

    def end_segment(ring):
        """the frame (and the ring) in one scatter: new[ring(k) ^ x] = (-1)^parity(ring(k) & z) old[k]; then the rescale"""
        nonlocal psi, N2, fx, fz
        dst = ring[None, :] ^ fx[:, None]
        sign = 1.0 - 2.0 * _parity(ring[None, :] & fz[:, None])
        new = np.empty_like(psi)
        new[rows, dst] = psi * sign
        small = N2 < 2.0 ** -200
        psi = np.where(small[:, None], new * 2.0 ** 100, new)
        N2 = np.where(small, N2 * 2.0 ** 200, N2)
        fx = np.zeros(M, np.int64)
        fz = np.zeros(M, np.int64)

    ring = ring_map(n)
    X = np.repeat(x, T, axis=0)
    call, col, s = 0, 0, 0
    for n_enc, ld in cfgs:
        assert n_enc == n
        for q in range(n):
            O._rx(psi, n, q, X[:, col + q])
            site1(ENC, q, words(call + q), nz['p1'][q])
        end_segment(kk)
        col += n
        call += n
        for _ in range(ld):
            for q in range(n):
                O._ry(psi, n, q, w[s, 0, q])
                O._rz(psi, n, q, w[s, 1, q])
                O._ry(psi, n, q, w[s, 2, q])
                site1(ROT, q, words(call + q), nz['p1'][q])
            call += n
            for j in range(n):
                c, t = (j + 1) % n, j
                fx ^= ((fx >> c) & 1) << t                               # the frame through CNOT(c -> t); the state stays
                fz ^= ((fz >> t) & 1) << c
                wd = words(call + 2 * j)
                err = wd[0] < np.uint64(NO.threshold(nz['p2'][j]))
                fired['pauli'] += int(err.sum())
                code = np.where(err, ((wd[1] * np.uint64(15)) >> np.uint64(32)).astype(np.int64) + 1, 0)
                for wire, p in ((c, code >> 2), (t, code & 3)):
                    bx, bz = pauli_bits(p, wire)
                    fx ^= bx
                    fz ^= bz
                relax(TGT, j, wd)
                relax(CTL, j, words(call + 2 * j + 1))
            call += 2 * n
            end_segment(ring)
            s += 1
    assert call == n_calls(n, cfgs)
    if counts is not None:
        counts.update(fired)
    pauli = O._check_pauli(ham_pauli, ham_diag)
    NO._basis_change(psi, n, pauli)
    prob = psi.real ** 2 + psi.imag ** 2
    tot = prob.sum(axis=1)
    r01, r10 = nz['readout01'], nz['readout10']
    if shots == 0:
        off, h = readout_weights(n, offset, coeff, ham_diag, r01, r10)
        vals = off + (prob @ h) / tot
    else:
        thr = [(np.uint64(NO.threshold(r01[i])), np.uint64(NO.threshold(r10[i]))) for i in range(n)]
        vals = NO.shot_values(prob / tot[:, None], words, call, n, lambda i, bit: np.where(bit == 1, thr[i][1], thr[i][0]), offset,
                              coeff, ham_diag)
    return vals.reshape(B, T)
