"""
numpy reference for the loss gradient under the calibrated device noise model (qhea_model_loss_grad_noisy_device_exact,
include/quanonet_hea.h), built on the literal model of tests/device_noise_reference.py: the timeline of a sub-layer slot by
slot, relaxation and depolarizing as Kraus operators, nothing folded into sites.

(i)   circuit_grad: the adjoint walk.  rho goes forward through the operations; the observable starts at O = B^dagger diag(h') B
      (h' under the per-bit confusion matrices) and is pulled back through the Kraus-form adjoint of every channel,
      O -> sum_K K^dagger O K; a rotation exp(-i theta sigma / 2) whose output state is rho_k gives d pred / d theta =
      Im Tr(O_k sigma rho_k).  inverse=False keeps rho after every rotation from the forward sweep; inverse=True walks rho
      back the way the kernel does, through the inverse of every channel -- formed here as the numerical inverse of the
      channel's superoperator matrix sum_K K (x) K*, not from the (off, a, b) algebra of the library.
(ii)  shift_grad: parameter shift through device_noise_reference.device_moments.  Every rotation is exp(-i theta sigma / 2)
      surrounded by linear maps, so d f / d theta = (f(theta + pi/2) - f(theta - pi/2)) / 2 exactly.
(iii) model_loss_grad: the model around the circuit, the [P + 2] buffer of the header (the chain rule of
      density_grad_reference.model_loss_grad).
(iv)  log10_amplification: the guard's log10 A_dev.
"""
import numpy as np

from oracle import hea_oracle as O
from tests import density_reference as DR
from tests import density_grad_reference as DGR
from tests import device_noise_reference as DNR


def _pairs():
    return [np.kron(a, b) for a in (DNR.I2,) + DNR.PAULIS for b in (DNR.I2,) + DNR.PAULIS]


def depolarizing2_kraus(p, dtype=np.complex128):
    """on (control, target): identity with weight 1 - p, each of the 15 other Pauli pairs p / 15"""
    p = DR.real_of(dtype)(p)
    ks = _pairs()
    return [np.sqrt(1.0 - p) * ks[0]] + [np.sqrt(p / 15.0) * k for k in ks[1:]]


def _superoperator_on(rho, n, wires, S):
    """the linear map with matrix S on (row bits, column bits) of the given wires: index (row, col) -> row * 2^m + col"""
    m = len(wires)
    St = S.reshape((2,) * (4 * m))                                       # out rows, out cols, in rows, in cols
    axes = [DR._row_axis(n, q) for q in wires] + [DR._col_axis(n, q) for q in wires]
    r = np.tensordot(St, rho, axes=(list(range(2 * m, 4 * m)), axes))
    return np.moveaxis(r, list(range(2 * m)), axes)


def _kraus_on(rho, n, wires, kraus, adjoint=False):
    """sum_K K rho K^dagger on the given wires (adjoint: sum_K K^dagger rho K); K is 2^m x 2^m, first wire most significant.
    The sum is taken over the operators first, sum_K K (x) K*, and applied to the row and column bits in one contraction."""
    ks = [K.conj().T for K in kraus] if adjoint else kraus
    return _superoperator_on(rho, n, wires, sum(np.kron(K, K.conj()) for K in ks))


def _inverse_on(rho, n, wires, kraus):
    """the inverse of the channel: its superoperator sum_K K (x) K* as a matrix on (row bits, column bits), inverted"""
    return _superoperator_on(rho, n, wires, np.linalg.inv(sum(np.kron(K, K.conj()) for K in kraus)))


def _relax_kraus(t, T1, T2, dtype=np.complex128):
    """amplitude damping then phase damping as one Kraus set (the products)"""
    return [P @ A for P in DNR.phase_damping_kraus(t, T1, T2, dtype) for A in DNR.amplitude_damping_kraus(t, T1, dtype)]


def _ops(n, cfgs, nz, dtype=np.complex128):
    """the timeline as a list: ('x' | 'y' | 'z', wire, angle key), ('ch', wires, kraus), ('cnot', control, target)"""
    ops, col, s = [], 0, 0

    def relax(q, t):
        return [('ch', (q,), _relax_kraus(t, nz['t1'][q], nz['t2'][q], dtype))] if t != 0.0 else []

    def dep1(q):
        return [('ch', (q,), DNR.depolarizing_kraus(nz['p1'][q], dtype))] if nz['p1'][q] != 0.0 else []

    for n_enc, ld in cfgs:
        assert n_enc == n
        for q in range(n):
            ops += [('x', q, ('x', col + q))] + dep1(q) + relax(q, nz['t_rx'])
        col += n
        for _ in range(ld):
            for q in range(n):
                ops += [('y', q, ('w', s, 0, q)), ('z', q, ('w', s, 1, q)), ('y', q, ('w', s, 2, q))] + dep1(q)
                ops += relax(q, nz['t_rot'])
            for j in range(n):
                ctl, tgt = (j + 1) % n, j
                ops.append(('cnot', ctl, tgt))
                if nz['p2'][j] != 0.0:
                    ops.append(('ch', (ctl, tgt), depolarizing2_kraus(nz['p2'][j], dtype)))
                for q in range(n):
                    if q in (ctl, tgt) or nz['idle']:
                        ops += relax(q, nz['t_cx'])
            s += 1
    return ops


def value_table(n, nz, offset=0.0, coeff=1.0, ham_diag=None, dtype=np.complex128):
    """h'[k] = sum_k' P(read k' | true k) h[k']: the expected read value of the true bitstring k"""
    real = DR.real_of(dtype)
    hv = DNR.value_table(n, offset, coeff, ham_diag, real)
    eye = np.eye(1 << n, dtype=real)
    return DNR.confuse(eye, n, nz['readout01'], nz['readout10']) @ hv


def _forward_sweep(n, ops, angle, B, dtype, keep=None):
    """rho from |0><0| through the timeline `ops` (every channel one superoperator contraction); keep: None, or the dict that
    receives rho after every rotation (the stored walk)"""
    rho = np.zeros((B,) + (2,) * (2 * n), dtype=dtype)
    rho[(slice(None),) + (0,) * (2 * n)] = 1.0
    for k, op in enumerate(ops):
        if op[0] == 'ch':
            rho = _kraus_on(rho, n, op[1], op[2])
        elif op[0] == 'cnot':
            rho = DGR._cnot(rho, n, op[1], op[2])
        else:
            rho = DR._gate(rho, n, op[1], DGR._rot(op[0], angle(op[2])))
            if keep is not None:
                keep[k] = rho
    return rho


def stored_final_rho(n, cfgs, x, w, nz, ham_pauli='Z', dtype=np.complex128):
    """rho[B, D, D] of device_noise_reference.final_rho by the stored walk's forward sweep: the same timeline in other
    arithmetic (a channel is the matrix sum_K K (x) K* on a wire's row and column bit, not a sum of K rho K^dagger)"""
    real = DR.real_of(dtype)
    x = np.asarray(x, real)
    w = np.asarray(w, real)
    B = x.shape[0]

    def angle(key):
        return x[:, key[1]] if key[0] == 'x' else np.full(B, w[key[1], key[2], key[3]])

    rho = _forward_sweep(n, _ops(n, cfgs, nz, dtype), angle, B, dtype)
    return np.ascontiguousarray(DR.basis_change(rho, n, ham_pauli)).reshape(B, 1 << n, 1 << n)


def circuit_grad(n, cfgs, x, w, nz, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', inverse=False, dtype=np.complex128):
    """
    (value[B], d value / d x [B, E], d value / d w [B, blk, 3, n]) of the exact expectation under the device noise (no bias).
    inverse=False: rho after every rotation is kept from the forward sweep; True: rho is walked back through inverse channels.
    dtype: np.complex128, or np.clongdouble for the stored walk in extended precision (density_reference.real_of; the inverse
    walk inverts its superoperators with LAPACK and stays fp64); the results come back in its real type.
    """
    pauli = O._check_pauli(ham_pauli, ham_diag)
    assert not inverse or np.dtype(dtype) == np.complex128, 'the inverse walk is fp64 only'
    real = DR.real_of(dtype)
    x = np.asarray(x, real)
    w = np.asarray(w, real)
    sq = DR.sq_of(dtype)
    B = x.shape[0]
    ops = _ops(n, cfgs, nz, dtype)

    def angle(key):
        return x[:, key[1]] if key[0] == 'x' else np.full(B, w[key[1], key[2], key[3]])

    keep = {}
    rho = _forward_sweep(n, ops, angle, B, dtype, None if inverse else keep)
    hv = value_table(n, nz, offset, coeff, ham_diag, dtype)
    obs = np.zeros((B,) + (2,) * (2 * n), dtype=dtype)
    obs.reshape(B, 1 << n, 1 << n)[:, np.arange(1 << n), np.arange(1 << n)] = hv
    if pauli != 'Z':
        for q in range(n):
            obs = DR._gate(obs, n, q, (sq, sq, sq, -sq))                             # H is its own dagger
            if pauli == 'Y':
                obs = DR._gate(obs, n, q, (1.0, 0.0, 0.0, 1j))                       # S = (S^dagger)^dagger
    value = np.real(DGR._trace(obs, rho, n))
    gx = np.zeros((B, x.shape[1]), dtype=real)
    gw = np.zeros((B,) + w.shape, dtype=real)
    for k in range(len(ops) - 1, -1, -1):
        op = ops[k]
        if op[0] == 'ch':
            if inverse:
                rho = _inverse_on(rho, n, op[1], op[2])
            obs = _kraus_on(obs, n, op[1], op[2], adjoint=True)
        elif op[0] == 'cnot':
            if inverse:
                rho = DGR._cnot(rho, n, op[1], op[2])
            obs = DGR._cnot(obs, n, op[1], op[2])
        else:
            if not inverse:
                rho = keep.pop(k)
            g = np.imag(DGR._trace(obs, DGR._left(rho, n, op[1], DGR.SIGMA[op[0]]), n))
            key = op[2]
            if key[0] == 'x':
                gx[:, key[1]] = g
            else:
                gw[:, key[1], key[2], key[3]] = g
            ud = DGR._dagger(DGR._rot(op[0], angle(key)))
            if inverse:
                rho = DR._gate(rho, n, op[1], ud)
            obs = DR._gate(obs, n, op[1], ud)
    return value, gx, gw


def shift_grad(n, cfgs, x, w, nz, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z'):
    """(value, gx, gw) as circuit_grad, by the two-term parameter-shift rule through device_noise_reference.device_moments"""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)

    def f(xx, ww):
        return DNR.device_moments(n, cfgs, xx, ww, nz, offset, coeff, ham_diag, ham_pauli)[0]

    value = f(x, w)
    gx = np.zeros_like(x)
    gw = np.zeros((x.shape[0],) + w.shape)
    for e in range(x.shape[1]):
        d = np.zeros_like(x)
        d[:, e] = np.pi / 2
        gx[:, e] = 0.5 * (f(x + d, w) - f(x - d, w))
    for idx in np.ndindex(w.shape):
        d = np.zeros_like(w)
        d[idx] = np.pi / 2
        gw[(slice(None),) + idx] = 0.5 * (f(x, w + d) - f(x, w - d))
    return value, gx, gw


def model_loss_grad(spec, flat, branch, trunk, y, nz, inv_batch_total, inverse=False, circuit=None, dtype=np.complex128):
    """
    ([P + 2] buffer, pred[B]) of the header's qhea_model_loss_grad_noisy_device_exact: gradients of sum_b (pred_b - y_b)^2 *
    inv_batch_total in the flat parameter layout, then sum (pred - y)^2 and sum y^2.  spec: density_grad_reference.spec_of.
    circuit: circuit_grad (default, with `inverse` and `dtype`) or shift_grad (fp64).  dtype: as in circuit_grad; with
    np.clongdouble the model around the circuit is done in the wide type too.
    """
    real = DR.real_of(dtype)
    y = np.asarray(y, np.float64).reshape(-1).astype(real)
    inv_batch_total = real(inv_batch_total)
    n, quanonet, cfgs, segs, tiles, off, off_ans, P, flat, x, w = DGR.model_circuit(spec, flat, branch, trunk, dtype)
    if circuit is None:
        value, gx, gw = circuit_grad(n, cfgs, x, w, nz, spec['offset'], spec['coeff'], spec['ham_diag'], spec['ham_pauli'],
                                     inverse=inverse, dtype=dtype)
    else:
        value, gx, gw = circuit(n, cfgs, x, w, nz, spec['offset'], spec['coeff'], spec['ham_diag'], spec['ham_pauli'])
    pred = value + (flat[0] if quanonet else 0.0)
    g = 2.0 * (pred - y) * inv_batch_total
    out = np.zeros(P + 2, dtype=real)
    if quanonet:
        out[0] = g.sum()
    out[off_ans:P] = np.einsum('b,bskq->skq', g, gw).reshape(-1)
    if spec['trainable']:
        col = 0
        for (name, _, cols), t in zip(segs, tiles):
            ow, ob = off[name]
            gcol = g[:, None] * gx[:, col:col + cols]
            out[ow:ow + cols] = (gcol * t).sum(axis=0)
            out[ob:ob + cols] = gcol.sum(axis=0)
            col += cols
    out[P] = ((pred - y) ** 2).sum()
    out[P + 1] = (y ** 2).sum()
    return out, pred


def site_tables(n, nz):
    """(chan [4, n, 3], lam2 [n]): the (off, a, b) triple of the four channel sites of every wire (ENC, ROT, CTL, TGT; the
    header's table), read off the composed Kraus channels with device_noise_reference.triple_of, and 16 p2[j] / 15"""
    chan = np.zeros((4, n, 3))
    for q in range(n):
        T1, T2, p = nz['t1'][q], nz['t2'][q], nz['p1'][q]
        idle = bool(nz['idle'])
        t_rot = nz['t_rot'] + ((q - 1) * nz['t_cx'] if idle and q >= 1 else 0.0)
        t_tgt = ((n - 1 if q == 0 else n - q) * nz['t_cx']) if idle else nz['t_cx']

        def gate_site(t):
            return lambda m: DNR.relax_1q(DNR.apply_1q(m, DNR.depolarizing_kraus(p)), t, T1, T2)
        chan[0, q] = DNR.triple_of(gate_site(nz['t_rx']))
        chan[1, q] = DNR.triple_of(gate_site(t_rot))
        chan[2, q] = DNR.triple_of(lambda m: DNR.relax_1q(m, nz['t_cx'], T1, T2))
        chan[3, q] = DNR.triple_of(lambda m: DNR.relax_1q(m, t_tgt, T1, T2))
    return chan, 16.0 * np.asarray(nz['p2'], np.float64) / 15.0


def log10_amplification(n, cfgs, nz, tables=None):
    """
    log10 A_dev = - sum log10 min(off, a) over the one-wire sites the circuit applies (ENC of a wire once per encoding layer,
    ROT / CTL / TGT once per sub-layer) - sum log10 (1 - lam_j) over its CNOT slots (once per sub-layer); inf for a singular
    channel (p1[q] >= 3/4, p2[j] >= 15/16, a site with min(off, a) = 0).  tables: (chan, lam2) of qhea_device_noise_tables;
    default site_tables(n, nz).
    """
    if any(p >= 0.75 for p in nz['p1']) or any(p >= 15.0 / 16.0 for p in nz['p2']):
        return np.inf
    chan, lam2 = site_tables(n, nz) if tables is None else tables
    blk = sum(ld for _, ld in cfgs)
    count = [len(cfgs), blk, blk, blk]
    total = 0.0
    for k in range(4):
        if count[k] == 0:
            continue
        for q in range(n):
            m = min(chan[k][q][0], chan[k][q][1])
            if not m > 0.0:
                return np.inf
            total -= count[k] * np.log10(m)
    if blk:
        total -= blk * float(np.sum(np.log10(1.0 - np.asarray(lam2))))
    return total
