"""
numpy reference for the sampled-trajectory loss gradient (qhea_model_loss_grad_noisy_wide, include/quanonet_hea.h).

For a fixed random stream a trajectory is an ideal circuit with fixed Pauli strings inserted, so its value is analytic in the
angles.  traj_grad replays the header's stream gate by gate (the draws and gates of tests/noise_oracle.py replay_values) while
recording what it applied, starts lambda = B^dagger diag(h') B psi (B: the basis change of an X / Y read-out, h' the readout-
folded weight) and walks the record back: a Pauli insertion is its own inverse, a rotation exp(-i theta sigma / 2) whose output
is psi_k contributes d value / d theta = Im<lambda_k|sigma|psi_k>.  traj_grad_shift differentiates the replay itself by central
differences at +- pi / 2, which for a rotation angle are exact (the parameter-shift rule), so the two forms agree to rounding.

The model around the circuit (frequency layers with their chain rule, the bias, the MSE residual, the flat [P + 2] layout) is
oracle.hea_oracle's own: its loss functions take an `engine`, and TrajEngine / ExactEngine are engines -- the mean over the T
trajectories of a row, and the exact noisy expectation of the density matrix (tests/density_reference.py exact_moments: what
noise_oracle.exact_values computes, without that routine's n <= 5 limit) with its derivative by the same central differences.
"""
import numpy as np

from oracle import hea_oracle as O
from tests import density_reference as DR
from tests import noise_oracle as NO

SQ = 1.0 / np.sqrt(2.0)


def _undo_basis_change(psi, n, pauli):
    """the dagger of noise_oracle._basis_change: H, then S for a Y read-out, on every wire"""
    if pauli == 'Z':
        return
    sq = 1.0 / np.sqrt(NO.real_of(psi.dtype)(2.0))
    for q in range(n):
        O._apply_1q(psi, n, q, sq, sq, sq, -sq)
        if pauli == 'Y':
            O._apply_1q(psi, n, q, 1.0, 0.0, 0.0, 1j)


def readout_table(diag, n, q, real=np.float64):
    """noise_oracle.readout_diag as one matrix product (that routine's 4^n terms in Python take seconds at n = 9): the same sum
    per entry, added by numpy; tests/test_noisy_traj_grad_reference.py holds the two together at n = 7.  Wire by wire (the same
    sum in another order, 2^n n terms) where `real` is wider than float64: a 4^n table in long double at n = 12 is too large."""
    if real is not np.float64:
        h, q = np.asarray(diag, np.float64).astype(real), real(q)
        kk = np.arange(1 << n)
        for i in range(n):
            h = (1 - q) * h + q * h[kk ^ (1 << i)]
        return h
    kk = np.arange(1 << n)
    conf = np.ones((1 << n, 1 << n))
    for i in range(n):
        conf *= np.where(((kk[:, None] ^ kk[None, :]) >> i) & 1, q, 1.0 - q)
    return conf @ np.asarray(diag, np.float64)


def readout_weights(n, offset, coeff, ham_diag, q, real=np.float64):
    """(off_term, h'[k]) of expectation mode, as noise_oracle._readout_weights"""
    if ham_diag is None:
        return NO._readout_weights(n, offset, coeff, None, q, real)
    return real(0.0) if real is not np.float64 else 0.0, readout_table(ham_diag, n, q, real)


def traj_grad(n, cfgs, x, w, noise, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', row0=0, dtype=np.complex128):
    """
    (value[B], d value / d x [B, E], d value / d w [B, blk, 3, n]), each the mean over the T = noise.trajectories trajectories of
    global row row0 + b on the stream of noise.seed (no bias): the adjoint walk per trajectory.  dtype: noise_oracle.real_of;
    the results come back in its real type.
    """
    assert noise.shots == 0
    real = NO.real_of(dtype)
    x = np.asarray(x, real)
    w = np.asarray(w, real)
    B, T = x.shape[0], int(noise.trajectories)
    words = NO.stream(B, T, row0, noise.seed)

    def draw(loc, p, two):
        wd = words(loc // 2)
        w0, w1 = wd[2 * (loc % 2)], wd[2 * (loc % 2) + 1]
        err = w0 < np.uint64(NO.threshold(p))
        idx = (w1 * np.uint64(15 if two else 3)) >> np.uint64(32)
        return err, idx.astype(np.int64)

    X = np.repeat(x, T, axis=0)
    M = B * T
    psi = np.zeros((M, 1 << n), dtype=dtype)
    psi[:, 0] = 1.0
    ops = []

    def insert(q, p, sel):
        if np.any(sel):
            NO._pauli(psi, n, q, p, sel)
            ops.append(('p', q, p, sel))

    loc, col, s = 0, 0, 0
    for n_enc, ld in cfgs:
        assert n_enc == n
        for q in range(n):
            NO._rx(psi, n, q, X[:, col + q])
            ops.append(('x', q, col + q))
            err, idx = draw(loc + q, noise.p1, False)
            for p in (1, 2, 3):
                insert(q, p, err & (idx == p - 1))
        col += n
        loc += n
        for _ in range(ld):
            for q in range(n):
                O._ry(psi, n, q, w[s, 0, q])
                ops.append(('y', q, (s, 0, q)))
                O._rz(psi, n, q, w[s, 1, q])
                ops.append(('z', q, (s, 1, q)))
                O._ry(psi, n, q, w[s, 2, q])
                ops.append(('y', q, (s, 2, q)))
                err, idx = draw(loc + q, noise.p1, False)
                for p in (1, 2, 3):
                    insert(q, p, err & (idx == p - 1))
            for j in range(n):
                c, t = (j + 1) % n, j
                O._cnot(psi, n, c, t)
                ops.append(('c', c, t))
                err, idx = draw(loc + n + j, noise.p2, True)
                code = idx + 1
                for p in (1, 2, 3):
                    insert(c, p, err & ((code >> 2) == p))
                    insert(t, p, err & ((code & 3) == p))
            loc += 2 * n
            s += 1
    assert loc == NO.n_locations(n, cfgs)
    pauli = O._check_pauli(ham_pauli, ham_diag)
    NO._basis_change(psi, n, pauli)
    off, h = readout_weights(n, offset, coeff, ham_diag, float(noise.readout), real)
    vals = off + (psi.real ** 2 + psi.imag ** 2) @ h
    lam = psi * h[None, :]
    _undo_basis_change(psi, n, pauli)
    _undo_basis_change(lam, n, pauli)
    gx = np.zeros((M, x.shape[1]), dtype=real)
    gw = np.zeros((M,) + w.shape, dtype=real)
    sigma = {'x': 'X', 'y': 'Y', 'z': 'Z'}
    rot = {'x': NO._rx, 'y': O._ry, 'z': O._rz}
    for op in reversed(ops):
        if op[0] == 'p':
            NO._pauli(psi, n, op[1], op[2], op[3])
            NO._pauli(lam, n, op[1], op[2], op[3])
        elif op[0] == 'c':
            O._cnot(psi, n, op[1], op[2])
            O._cnot(lam, n, op[1], op[2])
        else:
            g = O._im_inner_pauli(lam, psi, n, op[1], sigma[op[0]])
            if op[0] == 'x':
                gx[:, op[2]] = g
                ang = X[:, op[2]]
            else:
                gw[(slice(None),) + op[2]] = g
                ang = w[op[2]]
            rot[op[0]](psi, n, op[1], ang, dagger=True)
            rot[op[0]](lam, n, op[1], ang, dagger=True)
    mean = lambda a: a.reshape((B, T) + a.shape[1:]).mean(axis=1)
    return mean(vals), mean(gx), mean(gw)


def half_pi(real):
    """pi / 2 in the real type (np.pi / 2 for float64)"""
    return np.pi / 2 if real is np.float64 else 2 * np.arctan(real(1))


def _shift(value, x, w):
    """(value[B], d / d x [B, E], d / d w [B, blk, 3, n]) of value(x, w) -> [B] by central differences at +- pi / 2: exact
    where every angle enters through one rotation exp(-i theta sigma / 2).  In the type of x."""
    real = x.dtype.type
    hp = half_pi(real)
    gx, gw = np.zeros(x.shape, dtype=real), np.zeros((x.shape[0],) + w.shape, dtype=real)
    for e in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, e] += hp
        xm[:, e] -= hp
        gx[:, e] = 0.5 * (value(xp, w) - value(xm, w))
    for idx in np.ndindex(w.shape):
        wp, wm = w.copy(), w.copy()
        wp[idx] += hp
        wm[idx] -= hp
        gw[(slice(None),) + idx] = 0.5 * (value(x, wp) - value(x, wm))
    return value(x, w), gx, gw


def traj_grad_shift(n, cfgs, x, w, noise, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', row0=0, dtype=np.complex128,
                    weights=None):
    """traj_grad by central differences of noise_oracle.replay_values on the same stream.  weights: readout_weights of the
    call where the caller has them; without them a float64 replay makes noise_oracle's own, every time"""
    real = NO.real_of(dtype)
    if weights is None and real is not np.float64:
        weights = readout_weights(n, offset, coeff, ham_diag, float(noise.readout), real)
    val = lambda xx, ww: NO.replay_values(n, cfgs, xx, ww, noise, offset, coeff, ham_diag, ham_pauli, row0, dtype,
                                          weights).mean(axis=1)
    return _shift(val, np.asarray(x, real), np.asarray(w, real))


def exact_grad(n, cfgs, x, w, noise, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z'):
    """the exact noisy expectation per row (the CPU density matrix) and its derivatives by central differences"""
    val = lambda xx, ww: DR.exact_moments(n, cfgs, xx, ww, noise.p1, noise.p2, noise.readout, offset, coeff, ham_diag,
                                          ham_pauli)[0]
    return _shift(val, np.asarray(x, np.float64), np.asarray(w, np.float64))


class _Engine:
    """what oracle.hea_oracle's loss functions ask of an engine, over a circuit routine returning (value, d / d x, d / d w)"""

    def __init__(self, circuit):
        self._circuit, self._key, self._last = circuit, None, None

    def circuit(self, n, cfgs, x, w, *readout):
        """the loss functions ask for the forward and the backward of the same point: computed once"""
        key = (n, tuple(cfgs), np.asarray(x).tobytes(), np.asarray(w).tobytes(),
               tuple(np.asarray(v).tobytes() if isinstance(v, np.ndarray) else v for v in readout))
        if key != self._key:
            self._key, self._last = key, self._circuit(n, cfgs, x, w, *readout)
        return self._last

    def hea_forward(self, n, cfgs, x, w, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z'):
        return self.circuit(n, cfgs, x, w, offset, coeff, ham_diag, ham_pauli)[0]

    def hea_backward(self, n, cfgs, x, w, g, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z'):
        g = np.asarray(g, np.float64).reshape(-1)
        v, gx, gw = self.circuit(n, cfgs, x, w, offset, coeff, ham_diag, ham_pauli)
        return v, g[:, None] * gx, np.einsum('b,bskq->skq', g, gw)


def TrajEngine(noise, row0=0, form=traj_grad, dtype=np.complex128):
    """form: traj_grad or traj_grad_shift.  dtype: the form's; a wide engine goes with model_loss_grad(..., dtype=dtype)"""
    kw = {} if np.dtype(dtype) == np.complex128 else dict(dtype=dtype)
    return _Engine(lambda n, cfgs, x, w, off, co, hd, hp: form(n, cfgs, x, w, noise, off, co, hd, hp, row0, **kw))


def ExactEngine(noise):
    return _Engine(lambda n, cfgs, x, w, off, co, hd, hp: exact_grad(n, cfgs, x, w, noise, off, co, hd, hp))


def model_loss_grad(model, inputs, y, inv_batch_total, engine=None, dtype=np.complex128):
    """
    ([P + 2] buffer, pred[B]) of the header's calls for a QuanONetPT / HEAQNNPT (any device; the arithmetic is numpy): the
    gradients of sum_b (pred_b - y_b)^2 * inv_batch_total in model.parameters() order, then sum (pred - y)^2 and sum y^2.
    inputs: (branch, trunk) or (x,) as numpy arrays.  engine: TrajEngine / ExactEngine, or None for the ideal oracle.
    dtype: np.complex128 -- the model around the circuit is oracle.hea_oracle's, in float64 -- or np.clongdouble with an engine of
    that type: the frequency layers, the bias, the residual, the chain rule and the sums are then done in the wide type by
    tests/device_noise_grad_reference.py model_loss_grad (the same model and the same flat layout) around the engine's circuit.
    """
    if np.dtype(dtype) != np.complex128:
        from tests import density_grad_reference as DGR
        from tests import device_noise_grad_reference as DV
        flat = np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in model.parameters()])
        return DV.model_loss_grad(DGR.spec_of(model), flat, inputs[0], inputs[1] if len(inputs) > 1 else None, y, None, inv_batch_total,
                                  circuit=lambda n, cfgs, x, w, nz, *readout: engine.circuit(n, cfgs, x, w, *readout), dtype=dtype)
    from quanonet_amd.models import QuanONetPT
    q = model.quantum_layer
    n, net = model.num_qubits, tuple(model.net_size)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    names = [k for k, _ in model.named_parameters()]
    y = np.asarray(y, np.float64).reshape(-1)
    kw = dict(ham_bound=(q.ham_offset - q.ham_coeff * n, q.ham_offset + q.ham_coeff * n), batch_total=1.0 / inv_batch_total,
              ham_pauli=('Z', 'X', 'Y')[q.ham_pauli], ham_diag=q.ham_diag.detach().cpu().numpy() if q.use_full_ham else None,
              engine=engine)
    assert np.allclose(O.ham_params(n, *kw['ham_bound']), (q.ham_offset, q.ham_coeff), rtol=0, atol=1e-15)
    freq = model.branch_freq if isinstance(model, QuanONetPT) else model.freq
    if not hasattr(freq, 'weights'):
        kw['scale_coeff'] = float(freq.scale)
    if isinstance(model, QuanONetPT):
        loss, grads, pred = O.quanonet_loss_and_grads(sd, inputs[0], inputs[1], y, n, net, **kw)
    else:
        loss, grads, pred = O.heaqnn_loss_and_grads(sd, inputs[0], y, n, net, **kw)
    flat = np.concatenate([np.asarray(grads[k], np.float64).reshape(-1) for k in names])
    return np.concatenate([flat, [float(((pred - y) ** 2).sum()), float((y ** 2).sum())]]), pred


def dpred(model, inputs, engine):
    """d pred / d params of ONE row in model.parameters() order: with B = 1 and inv_batch_total = 1/2 the loss gradient is
    (pred - y) d pred / d params, so the gradients at y and y + 1 differ by it -- how the GPU tests read a row's derivative"""
    g0, _ = model_loss_grad(model, inputs, np.zeros(1), 0.5, engine)
    g1, _ = model_loss_grad(model, inputs, np.ones(1), 0.5, engine)
    return (g0 - g1)[:-2]
