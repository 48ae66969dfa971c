"""
CPU checks of noise-aware training (qhea_model_loss_grad_noisy_exact / qhea_model_train_steps_noisy_exact): the symbols, the
C ABI's argument checks and the conditioning guard (nothing is launched, no GPU needed), the numpy helper
tests/density_grad_reference.py against parameter shift through tests/density_reference.py, and the conditioning probe: the
inverse walk (what the kernel does) against the stored walk up to the guard's bound.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from tests import density_grad_reference as DG
from tests import density_reference as DR
from tests.conftest import ROOT
from tests.test_noisy_forward import _model

NEW = ('qhea_model_exact_noisy_grad_workspace_bytes', 'qhea_model_exact_noisy_log10_amplification',
       'qhea_model_loss_grad_noisy_exact', 'qhea_model_train_steps_noisy_exact')


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 520 and _lib.MIN_LIB_VERSION >= 520
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    for f in (_lib.model_loss_grad_noisy_exact, _lib.model_train_steps_noisy_exact, _lib.model_exact_noisy_log10_amplification):
        assert callable(f)
    from quanonet_amd.noise import amplification, exact_noisy_loss_and_grad
    assert callable(amplification) and callable(exact_noisy_loss_and_grad)


def _loss_grad(lib, d, batch, nz, ham_diag=None):
    """the call with every array NULL: what the checks in front of the pointers return"""
    return lib.qhea_model_loss_grad_noisy_exact(None if d is None else ctypes.byref(d), batch, None, None, None, None, ham_diag,
                                                None if nz is None else ctypes.byref(nz), 1.0, None, None, None, 0, None)


def _train_steps(lib, d, n_steps, nz, first_step=1):
    return lib.qhea_model_train_steps_noisy_exact(None if d is None else ctypes.byref(d), n_steps, None, None, None, None, None,
                                                  None, None if nz is None else ctypes.byref(nz), None, None, 0, None, None,
                                                  first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, 0, None)


def test_abi_argument_checks_without_gpu(lib):
    from quanonet_amd import _lib
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, 5, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0)
    P = _lib.model_param_count(d)
    # header, tables, pred and one record entry per row and angle (20 encoding columns + 4 sub-layers x 3 x 5 angles)
    fwd = lib.qhea_model_exact_noisy_workspace_bytes(ctypes.byref(d), 100)
    assert lib.qhea_model_exact_noisy_grad_workspace_bytes(ctypes.byref(d), 100) >= fwd + 100 * 8 + 100 * (20 + 60) * 8
    assert lib.qhea_model_exact_noisy_grad_workspace_bytes(ctypes.byref(d), -1) == 0
    assert lib.qhea_model_exact_noisy_grad_workspace_bytes(None, 100) == 0
    assert P == 1 + 2 * 20 + 60
    bad_desc = _lib.make_model_desc(_lib.MODEL_QUANONET, 5, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    bad_desc.n_qubits = 0
    assert lib.qhea_model_exact_noisy_grad_workspace_bytes(ctypes.byref(bad_desc), 100) == 0
    bads = (_lib.NoiseParams(-0.1, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.01, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
            _lib.NoiseParams(0, 0, float('nan'), 0, 1, 0), _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0),
            _lib.NoiseParams(0, float('nan'), 0, 0, 1, 0))
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    for call in (_loss_grad, _train_steps):
        assert call(lib, bad_desc, 10, ok) == -1
        assert call(lib, None, 10, ok) == -1
        assert call(lib, d, 0, ok) == 0                                           # empty batch / no steps
        for bad in bads:
            assert call(lib, d, 10, bad) == -1
            assert call(lib, d7, 10, bad) == -1                                   # bad rates are reported before the qubit count
        assert call(lib, d, 10, None) == -1                                       # no noise setting
        assert call(lib, d, 0, _lib.NoiseParams(0.01, 0.02, 0.03, -5, 0, 9)) == 0     # shots, trajectories, seed are ignored
        assert call(lib, d, -1, ok) == -1
        assert call(lib, d7, 10, ok) == -2
        assert call(lib, d, 10, ok) == -1                                         # valid up to the NULL arrays
    assert _train_steps(lib, d, 3, ok, first_step=0) == -1
    # X / Y read-outs do not combine with ham_diag (as in every other call)
    dx = _lib.make_model_desc(_lib.MODEL_QUANONET, 3, (1, 1, 1, 1), 4, 1, True, 0.1, 0.0, 1.0)
    dx.ham_pauli = 1
    assert _loss_grad(lib, dx, 10, ok, ham_diag=ctypes.cast(ctypes.c_void_p(256), ctypes.POINTER(ctypes.c_double))) == -1


def full_train_steps(lib, name, d, nz, n_steps=2, first_step=1, row_begin=True):
    """train-steps call `name` with every array present (host memory: the checks read row_begin and nothing else) and no
    workspace, so nothing is launched: the code that wins when the call has more than one fault"""
    from quanonet_amd import _lib
    P, rows = _lib.model_param_count(d), 5
    buf = lambda k: (ctypes.c_double * k)()
    rb = (ctypes.c_int64 * 3)(0, 3, rows) if row_begin else None
    return getattr(lib, name)(ctypes.byref(d), n_steps, rb, buf(rows * 8), buf(rows * 8), buf(rows), buf(P), None,
                              ctypes.byref(nz), buf(2), buf(2 * (P + 2)), P + 2, buf(P), buf(P), first_step, 1e-3, 0.9, 0.999,
                              1e-8, 0.0, None, 0, None)


def test_train_steps_two_faults_at_once(lib):
    """which code wins: first_step = 0 is refused with the descriptor, ahead of every other check of the call (the codes are
    those of the library before its entry points shared one body)"""
    from quanonet_amd import _lib
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, 5, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    ok, bad, singular = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0), _lib.NoiseParams(0, 1.01, 0, 0, 1, 0), _lib.NoiseParams(0.75, 0, 0, 0, 1, 0)
    name = 'qhea_model_train_steps_noisy_exact'
    table = [('first_step 0, no row_begin', dict(d=d, nz=ok, first_step=0, row_begin=False), -1),
             ('first_step 0, invalid rate', dict(d=d, nz=bad, first_step=0), -1),
             ('first_step 0, n = 7', dict(d=d7, nz=ok, first_step=0), -1),
             ('first_step 0, refused amplification', dict(d=d, nz=singular, first_step=0), -1),
             ('first_step 0, no steps', dict(d=d, nz=ok, first_step=0, n_steps=0), -1),
             ('n = 7 alone', dict(d=d7, nz=ok), -2),
             ('refused amplification alone', dict(d=d, nz=singular), -2),
             ('no workspace, a valid call of two steps', dict(d=d, nz=ok), -3)]
    for what, kw, want in table:
        assert full_train_steps(lib, name, **kw) == want, what


def _closed_form(n, E, blk, p1, p2):
    return -((E + n * blk) * math.log10(1 - 4 * p1 / 3) + n * blk * math.log10(1 - 16 * p2 / 15))


def test_guard(lib):
    from quanonet_amd import _lib
    amp = lambda d, nz: lib.qhea_model_exact_noisy_log10_amplification(ctypes.byref(d), ctypes.byref(nz))
    shapes = [(_lib.make_model_desc(_lib.MODEL_QUANONET, 5, (40, 2, 20, 2), 4, 1, True, 0.1, 0.0, 1.0), 5, 300, 120),
              (_lib.make_model_desc(_lib.MODEL_QUANONET, 5, (20, 2, 10, 2), 4, 1, False, 0.1, 0.0, 1.0), 5, 150, 60),
              (_lib.make_model_desc(_lib.MODEL_QUANONET, 2, (5, 1, 5, 1), 10, 1, True, 0.1, 0.0, 1.0), 2, 20, 10),
              (_lib.make_model_desc(_lib.MODEL_HEAQNN, 6, (3, 0), 4, 0, True, 0.1, 0.0, 1.0), 6, 18, 0),
              (_lib.make_model_desc(_lib.MODEL_HEAQNN, 9, (4, 3), 4, 0, True, 0.1, 0.0, 1.0), 9, 36, 12)]
    for d, n, E, blk in shapes:
        for p1, p2 in ((0.0, 0.0), (1e-3, 1e-2), (0.03, 0.08), (0.2, 0.5), (0.0, 0.3), (0.4, 0.0)):
            got = amp(d, _lib.NoiseParams(p1, p2, 0.3, 0, 1, 0))
            assert abs(got - _closed_form(n, E, blk, p1, p2)) <= 1e-12 * max(1.0, abs(got)), (n, E, blk, p1, p2)
    d = shapes[0][0]
    # the rates DESIGN 7f / 7g measure with: the headline shape is far inside the bound, the half-size one at half of it
    assert abs(amp(d, _lib.NoiseParams(1e-3, 1e-2, 1e-2, 0, 1, 0)) - 3.3) < 0.05
    assert abs(amp(shapes[1][0], _lib.NoiseParams(1e-3, 1e-2, 1e-2, 0, 1, 0)) - 1.65) < 0.03
    # singular channels
    for nz in (_lib.NoiseParams(0.75, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 15 / 16, 0, 0, 1, 0), _lib.NoiseParams(1, 1, 0, 0, 1, 0)):
        assert amp(d, nz) == math.inf
        assert _loss_grad(lib, d, 0, nz) == -2 and _train_steps(lib, d, 0, nz) == -2
    # bad input
    assert math.isnan(amp(d, _lib.NoiseParams(-0.1, 0, 0, 0, 1, 0)))
    assert math.isnan(lib.qhea_model_exact_noisy_log10_amplification(ctypes.byref(d), None))
    assert math.isnan(lib.qhea_model_exact_noisy_log10_amplification(None, ctypes.byref(_lib.NoiseParams(0, 0, 0, 0, 1, 0))))
    # just above the bound: refused (before the empty batch is looked at); just below: passes every check
    lo, hi = 0.0, 0.5
    for _ in range(200):                                                          # p2 with log10 A = 12 at p1 = p2 / 6
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _closed_form(5, 300, 120, mid / 6, mid) < 12.0 else (lo, mid)
    above, below = _lib.NoiseParams(hi * 1.001 / 6, hi * 1.001, 0, 0, 1, 0), _lib.NoiseParams(lo * 0.999 / 6, lo * 0.999, 0, 0, 1, 0)
    assert 12.0 < amp(d, above) < 12.05 and 11.95 < amp(d, below) < 12.0
    assert _loss_grad(lib, d, 0, above) == -2 and _train_steps(lib, d, 0, above) == -2
    assert _loss_grad(lib, d, 10, above) == -2
    assert _loss_grad(lib, d, 0, below) == 0 and _train_steps(lib, d, 0, below) == 0
    assert _loss_grad(lib, d, 10, below) == -1                                    # reaches the NULL arrays


def _shift(n, cfgs, x, w, p, kw):
    """(value, d value / d x, d value / d w) per row by parameter shift through density_reference.final_rho"""
    val = lambda xx, ww: DR.exact_moments(n, cfgs, xx, ww, *p, **kw)[0]
    sx, sw = np.zeros(x.shape), np.zeros((x.shape[0],) + w.shape)
    for e in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, e] += np.pi / 2
        xm[:, e] -= np.pi / 2
        sx[:, e] = 0.5 * (val(xp, w) - val(xm, w))
    for idx in np.ndindex(w.shape):
        wp, wm = w.copy(), w.copy()
        wp[idx] += np.pi / 2
        wm[idx] -= np.pi / 2
        sw[(slice(None),) + idx] = 0.5 * (val(x, wp) - val(x, wm))
    return val(x, w), sx, sw


@pytest.mark.parametrize('n', [2, 3, 4])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
@pytest.mark.parametrize('readout', ['Z', 'X', 'Y', 'diag'])
def test_helper_against_parameter_shift(n, kind, readout):
    """the whole [P + 2] buffer: circuit derivatives by parameter shift, the model around them by torch autograd"""
    from quanonet_amd.models import QuanONetPT
    p = (0.03, 0.08, 0.04)
    rows = 3
    rng = np.random.default_rng(10 * n + len(readout))
    for trainable in (True, False):
        m = _model(kind, n, trainable, readout, seed=n)
        if kind == 'quanonet':
            ins = (torch.tensor(rng.uniform(-1, 1, (rows, 3))), torch.tensor(rng.uniform(0, 1, (rows, 2))))
        else:
            ins = (torch.tensor(rng.uniform(-1, 1, (rows, 4))),)
        y = rng.normal(size=rows)
        spec = DG.spec_of(m)
        flat = torch.cat([q.detach().reshape(-1) for q in m.parameters()]).numpy()
        got, pred = DG.model_loss_grad(spec, flat, ins[0].numpy(), ins[1].numpy() if len(ins) > 1 else None, y, *p, 1.0 / 7)
        # the expected buffer: x as the modules compute it, shift-rule derivatives, chain rule by autograd
        if isinstance(m, QuanONetPT):
            x = torch.cat([m.trunk_freq(ins[1]), m.branch_freq(ins[0])], dim=1)
            cfgs, bias = O.block_configs_quanonet(n, m.net_size), m.bias
        else:
            x = m.freq(ins[0])
            cfgs, bias = O.block_configs_heaqnn(n, m.net_size), None
        qw = m.quantum_layer.ansatz_weights
        kw = dict(offset=spec['offset'], coeff=spec['coeff'], ham_diag=spec['ham_diag'], ham_pauli=spec['ham_pauli'])
        v, sx, sw = _shift(n, cfgs, x.detach().numpy(), qw.detach().numpy(), p, kw)
        ref_pred = v + (float(bias.item()) if bias is not None else 0.0)
        np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=1e-12)
        g = torch.tensor(2.0 * (ref_pred - y) / 7)
        surrogate = (g[:, None] * torch.tensor(sx) * x).sum() + (torch.einsum('b,bskq->skq', g, torch.tensor(sw)) * qw).sum()
        if bias is not None:
            surrogate = surrogate + g.sum() * bias.sum()
        for q in m.parameters():
            q.grad = None
        surrogate.backward()
        ref = np.concatenate([(q.grad if q.grad is not None else torch.zeros_like(q)).reshape(-1).numpy() for q in m.parameters()]
                             + [np.array([((ref_pred - y) ** 2).sum(), (y ** 2).sum()])])
        assert got.shape == ref.shape
        print(f'n={n} {kind} {readout} trainable={trainable}: max|err|={np.abs(got - ref).max():.2e} max|g|={np.abs(ref).max():.2e}')
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)


def _rates_for(n, E, blk, target):
    """(p1, p2 = 6 p1) with log10 A = target"""
    if target == 0.0:
        return 0.0, 0.0
    lo, hi = 0.0, 0.9
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _closed_form(n, E, blk, mid / 6, mid) < target else (lo, mid)
    return lo / 6, lo


@pytest.mark.parametrize('n,blocks,ld', [(5, 30, 2), (5, 60, 2), (6, 10, 2)])
def test_conditioning_probe(n, blocks, ld):
    """
    The kernel walks rho back through inverse channels; the helper's stored walk never inverts anything.  Their difference over
    log10 A = 0 .. 12 (the guard's bound) at the depths users run -- 60 and 120 sub-layers at n = 5 (Q5 Net20-2-10-2 and
    Net40-2-20-2), 20 at n = 6 -- measures what the inversion costs: at most 1e-12 is accepted; 6.3e-15 was measured at A = 1 (gradients of order 1),
    4e-16 beyond (the gradients shrink with 1 / A).
    """
    rng = np.random.default_rng(n + blocks)
    cfgs = [(n, ld)] * blocks
    E, blk = n * blocks, blocks * ld
    x = rng.uniform(-np.pi, np.pi, (1, E))
    w = rng.uniform(-np.pi, np.pi, (blk, 3, n))
    for target in (0.0, 4.0, 8.0, 11.99):
        p1, p2 = _rates_for(n, E, blk, target)
        logA = DG.log10_amplification(n, cfgs, p1, p2)
        assert abs(logA - target) < 1e-6 and logA <= 12.0
        v0, gx0, gw0 = DG.circuit_grad(n, cfgs, x, w, p1, p2, 0.01, coeff=5.0 / n)
        v1, gx1, gw1 = DG.circuit_grad(n, cfgs, x, w, p1, p2, 0.01, coeff=5.0 / n, inverse=True)
        err = max(np.abs(gx0 - gx1).max(), np.abs(gw0 - gw1).max(), np.abs(v0 - v1).max())
        print(f'n={n} sub-layers={blk} p1={p1:.4g} p2={p2:.4g} log10A={logA:.2f}: inverse walk - stored walk = {err:.2e}, '
              f'max|g|={max(np.abs(gx0).max(), np.abs(gw0).max()):.2e}')
        assert err <= 1e-12
