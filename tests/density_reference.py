"""
n-general density-matrix reference for the exact noisy forward (qhea_model_forward_noisy_exact, include/quanonet_hea.h):
exact_moments returns what tests/noise_oracle.py exact_values returns -- the exact expectation of a read value under the
header's channels and the variance of one shot -- without that routine's n <= 5 limit, so that n = 6 has a reference too.

rho is kept as a tensor of 2n two-level axes per row, rho[b, r_{n-1}, ..., r_0, c_{n-1}, ..., c_0] (little-endian wires as in
oracle.hea_oracle), gates act as U on a row axis and U* on the column axis, and the depolarizing channels are applied in their
closed computational-basis forms instead of the oracle's sums over Pauli strings:
  * one qubit, wire q: elements whose row and column bit of q differ are scaled by 1 - 4p/3; the two with equal bits become
    (1 - 2p/3) itself + (2p/3) the other;
  * two qubits (c, t), lam = 16p/15: elements whose row bits (c, t) differ from their column bits are scaled by 1 - lam; each
    of the four with equal bits becomes (1 - lam) itself + (lam / 4) the sum of the four.
tests/test_exact_noisy_abi.py checks this routine against exact_values at n = 2..5.
"""
import numpy as np

from oracle import hea_oracle as O

SQ = 1.0 / np.sqrt(2.0)


def real_of(dtype):
    """the real scalar type of a complex dtype (np.complex128 -> np.float64, np.clongdouble -> np.longdouble).  Every routine
    here and in the gradient helpers takes dtype=np.complex128 by default; with np.clongdouble the inputs stay the float64 data
    they are and everything computed from them -- half angles, sin / cos / exp, channel coefficients, sums -- is done in the
    wide type (tests/density_precision_cases.py)."""
    return np.finfo(dtype).dtype.type


def sq_of(dtype):
    """1 / sqrt 2 in the real type of dtype (SQ for complex128)"""
    return 1.0 / np.sqrt(real_of(dtype)(2.0))


def _row_axis(n, q):
    return 1 + (n - 1 - q)


def _col_axis(n, q):
    return 1 + n + (n - 1 - q)


def _gate(rho, n, q, m):
    """rho <- M_q rho M_q^dagger; m = (m00, m01, m10, m11), each a scalar or a (B,) array"""
    B = rho.shape[0]
    u = np.empty((B, 2, 2), dtype=rho.dtype)
    u[:, 0, 0], u[:, 0, 1], u[:, 1, 0], u[:, 1, 1] = m
    r = np.moveaxis(rho, _row_axis(n, q), 1)
    r = np.einsum('bij,bj...->bi...', u, r)
    rho = np.moveaxis(r, 1, _row_axis(n, q))
    c = np.moveaxis(rho, _col_axis(n, q), 1)
    c = np.einsum('bij,bj...->bi...', np.conj(u), c)
    return np.moveaxis(c, 1, _col_axis(n, q))


def _depolarize1(rho, n, q, p):
    if p == 0.0:
        return rho
    r = np.moveaxis(rho, (_row_axis(n, q), _col_axis(n, q)), (1, 2)).copy()
    d0, d1 = r[:, 0, 0].copy(), r[:, 1, 1].copy()
    r[:, 0, 1] *= 1.0 - 4.0 * p / 3.0
    r[:, 1, 0] *= 1.0 - 4.0 * p / 3.0
    r[:, 0, 0] = (1.0 - 2.0 * p / 3.0) * d0 + (2.0 * p / 3.0) * d1
    r[:, 1, 1] = (1.0 - 2.0 * p / 3.0) * d1 + (2.0 * p / 3.0) * d0
    return np.moveaxis(r, (1, 2), (_row_axis(n, q), _col_axis(n, q)))


def _cnot_depolarize2(rho, n, c, t, p):
    """CNOT(c -> t) on both sides, then two-qubit depolarizing on (c, t)"""
    axes = (_row_axis(n, c), _row_axis(n, t), _col_axis(n, c), _col_axis(n, t))
    r = np.moveaxis(rho, axes, (1, 2, 3, 4)).copy()
    r[:, 1] = r[:, 1, ::-1].copy()                       # row side: control = 1 flips the target
    r[:, :, :, 1] = r[:, :, :, 1, ::-1].copy()           # column side
    if p != 0.0:
        lam = 16.0 * p / 15.0
        pairs = [(a, b) for a in (0, 1) for b in (0, 1)]
        eq = [r[:, a, b, a, b].copy() for a, b in pairs]
        tot = eq[0] + eq[1] + eq[2] + eq[3]
        r *= 1.0 - lam
        for v, (a, b) in zip(eq, pairs):
            r[:, a, b, a, b] = (1.0 - lam) * v + (lam / 4.0) * tot
    return np.moveaxis(r, (1, 2, 3, 4), axes)


def final_rho(n, cfgs, x, w, p1, p2, ham_pauli='Z', dtype=np.complex128):
    """rho[B, D, D] after the circuit, its channels and the noiseless basis change of the X / Y read-outs"""
    real = real_of(dtype)
    x = np.asarray(x, real)
    w = np.asarray(w, real)
    p1, p2 = real(p1), real(p2)
    B, D = x.shape[0], 1 << n
    rho = np.zeros((B,) + (2,) * (2 * n), dtype=dtype)
    rho[(slice(None),) + (0,) * (2 * n)] = 1.0
    col, s = 0, 0
    for n_enc, ld in cfgs:
        assert n_enc == n
        for q in range(n):
            c, sn = np.cos(x[:, col + q] / 2), np.sin(x[:, col + q] / 2)
            rho = _gate(rho, n, q, (c, -1j * sn, -1j * sn, c))
            rho = _depolarize1(rho, n, q, p1)
        col += n
        for _ in range(ld):
            for q in range(n):
                for ang, kind in ((w[s, 0, q], 'y'), (w[s, 1, q], 'z'), (w[s, 2, q], 'y')):
                    c, sn = np.cos(ang / 2), np.sin(ang / 2)
                    if kind == 'y':
                        rho = _gate(rho, n, q, (c, -sn, sn, c))
                    else:
                        rho = _gate(rho, n, q, (np.exp(-0.5j * ang), 0.0, 0.0, np.exp(0.5j * ang)))
                rho = _depolarize1(rho, n, q, p1)
            for j in range(n):
                rho = _cnot_depolarize2(rho, n, (j + 1) % n, j, p2)
            s += 1
    return np.ascontiguousarray(basis_change(rho, n, ham_pauli)).reshape(B, D, D)


def basis_change(rho, n, ham_pauli):
    """the noiseless basis change of an X / Y read-out on rho[B, 2, .., 2]: H (X) or H S^dagger (Y) on every wire"""
    if ham_pauli != 'Z':
        sq = sq_of(rho.dtype)
        for q in range(n):
            if ham_pauli == 'Y':
                rho = _gate(rho, n, q, (1.0, 0.0, 0.0, -1j))
            rho = _gate(rho, n, q, (sq, sq, sq, -sq))
    return rho


def exact_moments(n, cfgs, x, w, p1, p2, readout, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', dtype=np.complex128):
    """(mean, var) per row, no bias: the exact expectation of a read value and the variance of one shot's value"""
    pauli = O._check_pauli(ham_pauli, ham_diag)
    rho = final_rho(n, cfgs, x, w, float(p1), float(p2), pauli, dtype)
    return moments_of(np.real(np.einsum('bkk->bk', rho)), n, readout, offset, coeff, ham_diag)


def moments_of(prob, n, readout, offset=0.0, coeff=1.0, ham_diag=None):
    """exact_moments' read-out on outcome probabilities prob[B, 2^n] = diag rho, in prob's type: the confusion applied to the
    probabilities, the sums as matrix products"""
    real = prob.dtype.type
    readout = real(readout)
    D = 1 << n
    kk = np.arange(D)
    conf = np.ones((D, D), dtype=real)
    for i in range(n):
        diff = ((kk[:, None] ^ kk[None, :]) >> i) & 1
        conf *= np.where(diff, readout, 1.0 - readout)
    pread = prob @ conf
    if ham_diag is not None:
        hv = np.asarray(ham_diag, np.float64).astype(real)
    else:
        pop = sum((kk >> i) & 1 for i in range(n))
        hv = real(offset) + real(coeff) * (n - 2.0 * pop)
    mean = pread @ hv
    var = pread @ (hv * hv) - mean ** 2
    return mean, var
