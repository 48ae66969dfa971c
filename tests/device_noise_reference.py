"""
Numpy reference for the exact noisy forward under the calibrated device noise model (qhea_device_noise,
qhea_model_forward_noisy_device_exact; include/quanonet_hea.h).  It is a literal statement of the model and follows the timeline
of a sub-layer step by step:
  * relaxation as Kraus operators: amplitude damping with gamma = 1 - exp(-t / T1), then phase damping with the pure-dephasing
    factor exp(-t / T2) / sqrt(1 - gamma);
  * depolarizing as the Pauli mixture (one qubit: X, Y, Z each p / 3; two qubits: each of the 15 non-identity pairs p / 15);
  * the idle relaxation applied slot by slot to every wire that is not in the slot's CNOT -- nothing is folded into sites;
  * the readout error as a 2 x 2 confusion matrix per bit applied to the outcome probabilities.
It uses none of the (off, a, b) algebra of the library, so it checks the host's folding as well as the kernel.  rho is kept in
the layout of tests/density_reference.py.
"""
import numpy as np

from tests import density_reference as DR

I2 = np.eye(2, dtype=np.complex128)
PX = np.array([[0, 1], [1, 0]], dtype=np.complex128)
PY = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
PZ = np.array([[1, 0], [0, -1]], dtype=np.complex128)
PAULIS = (PX, PY, PZ)


def amplitude_damping_kraus(t, T1, dtype=np.complex128):
    """dtype (here and below): the operators' type; t, T1, T2 and p are float64 data, what is computed from them -- gamma, the
    factors, the square roots -- is computed in its real type (density_reference.real_of)"""
    real = DR.real_of(dtype)
    t, T1 = real(t), real(T1)
    gamma = 1.0 - np.exp(-t / T1) if np.isfinite(T1) else real(0.0)
    return [np.array([[1, 0], [0, np.sqrt(1.0 - gamma)]], dtype=dtype),
            np.array([[0, np.sqrt(gamma)], [0, 0]], dtype=dtype)]


def phase_damping_kraus(t, T1, T2, dtype=np.complex128):
    """pure dephasing on top of amplitude damping: the off-diagonals end at exp(-t / T2) in total"""
    real = DR.real_of(dtype)
    t, T1, T2 = real(t), real(T1), real(T2)
    gamma = 1.0 - np.exp(-t / T1) if np.isfinite(T1) else real(0.0)
    total = np.exp(-t / T2) if np.isfinite(T2) else real(1.0)
    f = total / np.sqrt(1.0 - gamma) if gamma < 1.0 else real(0.0)
    f = min(f, real(1.0))                                                # T2 = 2 T1 to rounding
    return [np.sqrt((1.0 + f) / 2.0) * I2, np.sqrt((1.0 - f) / 2.0) * PZ]


def depolarizing_kraus(p, dtype=np.complex128):
    p = DR.real_of(dtype)(p)
    return [np.sqrt(1.0 - p) * I2] + [np.sqrt(p / 3.0) * P for P in PAULIS]


def apply_1q(rho2, kraus):
    """a channel on a single qubit's 2 x 2 matrix"""
    return sum(K @ rho2 @ K.conj().T for K in kraus)


def relax_1q(rho2, t, T1, T2):
    return apply_1q(apply_1q(rho2, amplitude_damping_kraus(t, T1)), phase_damping_kraus(t, T1, T2))


def triple_of(channel):
    """(off, a, b) of a phase-covariant single-qubit map given as a function of a 2 x 2 matrix: the factor of the off-diagonal
    elements and z' = a z + b tr, read off the images of |0><1|, Z and the identity"""
    e01 = np.array([[0, 1], [0, 0]], dtype=np.complex128)
    off = channel(e01)[0, 1]
    zi, zz = channel(I2.copy()), channel(PZ.copy())
    b = (zi[0, 0] - zi[1, 1]) / 2.0
    a = (zz[0, 0] - zz[1, 1]) / 2.0
    assert abs(off.imag) < 1e-15 and abs(a.imag) < 1e-15 and abs(b.imag) < 1e-15
    return np.array([off.real, a.real, b.real])


def _unitary(rho, n, q, m):
    """U rho U^dagger on wire q; m = (u00, u01, u10, u11), each a scalar or one value per row"""
    B = rho.shape[0]
    u = np.empty((B, 2, 2), dtype=rho.dtype)
    u[:, 0, 0], u[:, 0, 1], u[:, 1, 0], u[:, 1, 1] = m
    for ax, mat in ((DR._row_axis(n, q), u), (DR._col_axis(n, q), np.conj(u))):
        r = np.moveaxis(rho, ax, 1)
        shape = r.shape
        rho = np.moveaxis(np.matmul(mat, r.reshape(B, 2, -1)).reshape(shape), 1, ax)
    return rho


def _op(rho, n, q, K):
    """K rho K^dagger on wire q for one 2 x 2 matrix K, the same for every row"""
    ra, ca = DR._row_axis(n, q), DR._col_axis(n, q)
    r = np.moveaxis(np.tensordot(K, rho, axes=(1, ra)), 0, ra)
    return np.moveaxis(np.tensordot(K.conj(), r, axes=(1, ca)), 0, ca)


def _kraus(rho, n, q, kraus):
    return sum(_op(rho, n, q, K) for K in kraus)


_pauli = _op


def _relax(rho, n, q, t, nz):
    if t == 0.0:
        return rho
    rho = _kraus(rho, n, q, amplitude_damping_kraus(t, nz['t1'][q], rho.dtype))
    return _kraus(rho, n, q, phase_damping_kraus(t, nz['t1'][q], nz['t2'][q], rho.dtype))


def _depolarize1(rho, n, q, p):
    if p == 0.0:
        return rho
    p = DR.real_of(rho.dtype)(p)
    return (1.0 - p) * rho + (p / 3.0) * sum(_pauli(rho, n, q, P) for P in PAULIS)


def _depolarize2(rho, n, c, t, p):
    """(1 - p) rho + p / 15 sum over the 15 non-identity pairs: the sum over all 16 pairs, wire by wire, minus the identity's term"""
    if p == 0.0:
        return rho
    p = DR.real_of(rho.dtype)(p)
    over_t = rho + sum(_pauli(rho, n, t, P) for P in PAULIS)
    over_both = over_t + sum(_pauli(over_t, n, c, P) for P in PAULIS)
    return (1.0 - p) * rho + (p / 15.0) * (over_both - rho)


def final_rho(n, cfgs, x, w, nz, ham_pauli='Z', dtype=np.complex128):
    """rho[B, D, D] after the circuit under the device noise `nz` (a dict: p1, p2, readout01, readout10, t1, t2 as length-n
    sequences, t_rx, t_rot, t_cx, idle) and the noiseless basis change of the X / Y read-outs"""
    real = DR.real_of(dtype)
    x = np.asarray(x, real)
    w = np.asarray(w, real)
    B, D = x.shape[0], 1 << n
    rho = np.zeros((B,) + (2,) * (2 * n), dtype=dtype)
    rho[(slice(None),) + (0,) * (2 * n)] = 1.0
    col, s = 0, 0
    for n_enc, ld in cfgs:
        assert n_enc == n
        for q in range(n):                                               # the encoding layer: all wires at once, t_rx
            c, sn = np.cos(x[:, col + q] / 2), np.sin(x[:, col + q] / 2)
            rho = _unitary(rho, n, q, (c, -1j * sn, -1j * sn, c))
            rho = _depolarize1(rho, n, q, nz['p1'][q])
            rho = _relax(rho, n, q, nz['t_rx'], nz)
        col += n
        for _ in range(ld):
            for q in range(n):                                           # the rotation layer: the fused RY RZ RY, t_rot
                for ang, kind in ((w[s, 0, q], 'y'), (w[s, 1, q], 'z'), (w[s, 2, q], 'y')):
                    c, sn = np.cos(ang / 2), np.sin(ang / 2)
                    if kind == 'y':
                        rho = _unitary(rho, n, q, (c, -sn, sn, c))
                    else:
                        rho = _unitary(rho, n, q, (np.exp(-0.5j * ang), 0.0, 0.0, np.exp(0.5j * ang)))
                rho = _depolarize1(rho, n, q, nz['p1'][q])
                rho = _relax(rho, n, q, nz['t_rot'], nz)
            for j in range(n):                                           # slot j, t_cx
                ctl, tgt = (j + 1) % n, j
                rho = DR._cnot_depolarize2(rho, n, ctl, tgt, 0.0)
                rho = _depolarize2(rho, n, ctl, tgt, nz['p2'][j])
                for q in range(n):
                    if q in (ctl, tgt) or nz['idle']:
                        rho = _relax(rho, n, q, nz['t_cx'], nz)
            s += 1
    return np.ascontiguousarray(basis_change(rho, n, ham_pauli)).reshape(B, D, D)


def basis_change(rho, n, ham_pauli):
    """the noiseless basis change of an X / Y read-out on rho[B, 2, .., 2], with this file's _unitary"""
    if ham_pauli != 'Z':
        sq = DR.sq_of(rho.dtype)
        for q in range(n):
            if ham_pauli == 'Y':
                rho = _unitary(rho, n, q, (1.0, 0.0, 0.0, -1j))
            rho = _unitary(rho, n, q, (sq, sq, sq, -sq))
    return rho


def confuse(prob, n, readout01, readout10):
    """outcome probabilities [B, 2^n] -> probabilities of the read bitstrings: per bit q the matrix
    [[1 - r01, r10], [r01, 1 - r10]] (column = the true bit, row = the read bit), in prob's type"""
    B = prob.shape[0]
    real = prob.dtype.type
    p = prob.reshape((B,) + (2,) * n)                                    # axis 1 + (n - 1 - q) is bit q
    for q in range(n):
        r01, r10 = real(readout01[q]), real(readout10[q])
        m = np.array([[1.0 - r01, r10], [r01, 1.0 - r10]])
        ax = 1 + (n - 1 - q)
        p = np.moveaxis(np.tensordot(m, np.moveaxis(p, ax, 0), axes=(1, 0)), 0, ax)
    return p.reshape(B, 1 << n)


def value_table(n, offset=0.0, coeff=1.0, ham_diag=None, real=np.float64):
    if ham_diag is not None:
        return np.asarray(ham_diag, np.float64).astype(real)
    kk = np.arange(1 << n)
    return real(offset) + real(coeff) * (n - 2.0 * sum((kk >> i) & 1 for i in range(n)))


def device_moments(n, cfgs, x, w, nz, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', dtype=np.complex128):
    """(mean, var) per row, no bias: the expectation of a read value and the variance of one shot's value"""
    rho = final_rho(n, cfgs, x, w, nz, ham_pauli, dtype)
    return moments_of(np.real(np.einsum('bkk->bk', rho)), n, nz, offset, coeff, ham_diag)


def moments_of(prob, n, nz, offset=0.0, coeff=1.0, ham_diag=None):
    """device_moments' read-out on outcome probabilities prob[B, 2^n] = diag rho, in prob's type"""
    pread = confuse(prob, n, nz['readout01'], nz['readout10'])
    hv = value_table(n, offset, coeff, ham_diag, prob.dtype.type)
    mean = pread @ hv
    return mean, pread @ (hv * hv) - mean ** 2
