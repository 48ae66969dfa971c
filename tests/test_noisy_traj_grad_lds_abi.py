"""
The sampled-trajectory gradient at n = 10..12 on the GPU (qhea_model_loss_grad_noisy_lds / qhea_model_train_steps_noisy_lds,
through quanonet_amd._lib) against the numpy reference tests/noisy_traj_grad_reference.py, which replays the header's random
stream: the whole [P + 2] buffer and pred at n = 10, 11, 12 over the axis combinations of tests/test_noisy_traj_grad_abi.py,
noiseless = the ideal call, pred = the forward call's, independence of the batch, train_steps = the loop of single calls,
refusals, graph capture.
Tolerance against the reference: atol 1e-10, the one the HIP path is held to against the oracle.
Shapes: two blocks per net, sub-layers per block 1 and 2 (tests/test_noisy_traj_grad_reference.py build); the kernel's tile is
2 trajectories, so T = 1, 2 and 3 are one short tile, one full tile, and a full tile followed by a tile of one (the n = 7..9
cases' T = 1, 4, 5 mapped to this tile).  n = 10 and 11 run three gate qubits per pass (a ragged last pass each), n = 12 four.
No unbiasedness check here: the exact derivative would need a 4^10-entry density matrix on the CPU; the estimator is the one
tests/test_noisy_traj_grad_abi.py checks at n = 7, what is new is the walk, which the reference comparison pins.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import noisy_traj_grad_reference as TG
from tests.test_noisy_traj_grad_abi import ATOL, BIG, CASES, _adam_state, _diag, _on
from tests.test_noisy_traj_grad_reference import build, inputs, noise_model

pytestmark = pytest.mark.gpu
NS = [10, 11, 12]
TILE = 2


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _call(m, ins, y, nz, row0=0, inv=None, want_pred=True):
    """(grad[P+2], pred[B]) of one qhea_model_loss_grad_noisy_lds call as numpy arrays; m, ins, y on the device"""
    from quanonet_amd import _lib
    flat = H.flat(m)
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device) if want_pred else None
    _lib.model_loss_grad_noisy_lds(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat, nz.params(),
                                   1.0 / rows if inv is None else inv, grad, row0=row0, ham_diag=_diag(m), pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (pred.cpu().numpy() if want_pred else None)


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('case', range(len(CASES)))
def test_against_the_reference(dev, n, case):
    kind, trainable, readout, q, row0, T, (p1, p2) = CASES[case]
    T = {1: 1, 4: TILE, 5: TILE + 1}[T]                       # one trajectory, a full tile, a full tile and one more
    rows = 3
    cpu = build(kind, n, trainable, readout, seed=n + case, net=(2, 1) if case == 4 else None)
    ins, y = inputs(kind, rows, seed=case), np.random.default_rng(n + case).normal(scale=0.7, size=rows)
    nz = noise_model((p1, p2, q), T=T, seed=1234 + case)
    ref, ref_pred = TG.model_loss_grad(cpu, ins, y, 1.0 / 7, TG.TrajEngine(nz, row0))
    grad, pred = _call(cpu.to(dev), *_on(dev, ins, y), nz, row0=row0, inv=1.0 / 7)
    tag = f'n={n} {kind} trainable={trainable} {readout} q={q} row0={row0} T={T} p=({p1}, {p2})'
    print(f'{tag}: max|grad err|={np.abs(grad - ref).max():.2e} max|pred err|={np.abs(pred - ref_pred).max():.2e} '
          f'max|grad|={np.abs(ref[:-2]).max():.2e}')
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL, err_msg=tag)


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_noiseless_equals_ideal(dev, n, kind):
    from quanonet_amd import _lib
    for trainable, readout in ((True, 'Z'), (False, 'X'), (True, 'Y'), (False, 'diag')):
        m = build(kind, n, trainable, readout, seed=n).to(dev)
        rows = 7
        ins, y = _on(dev, inputs(kind, rows, seed=rows), np.random.default_rng(rows).normal(size=rows))
        grad, pred = _call(m, ins, y, noise_model((0.0, 0.0, 0.0), T=1, seed=3), row0=11)
        flat = H.flat(m)
        ideal = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=dev)
        ipred = torch.zeros(rows, dtype=torch.float64, device=dev)
        _lib.model_loss_grad(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat, 1.0 / rows, ideal,
                             ham_diag=_diag(m), pred=ipred)
        torch.cuda.synchronize()
        tag = f'n={n} {kind} trainable={trainable} {readout}'
        np.testing.assert_allclose(grad, ideal.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)
        np.testing.assert_allclose(pred, ipred.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)


@pytest.mark.parametrize('n,kind,readout', [(10, 'quanonet', 'Z'), (11, 'heaqnn', 'diag'), (12, 'quanonet', 'X'), (11, 'heaqnn', 'Y')])
def test_pred_is_the_forward_calls(dev, n, kind, readout):
    """same noise and row0: the two calls add the same trajectory values in different tiles (and at n = 10, 11 in groups of 8
    basis states where the forward has 16); the bound is the one the n = 7..9 call's pred is held to (1e-13)"""
    from quanonet_amd import _lib
    m = build(kind, n, True, readout, seed=n).to(dev)
    rows = 9
    ins, y = _on(dev, inputs(kind, rows, seed=2), np.zeros(rows))
    for T, row0 in ((1, 0), (TILE + 1, BIG), (100, 5)):
        nz = noise_model((0.03, 0.08, 0.04), T=T, seed=77)
        _, pred = _call(m, ins, y, nz, row0=row0)
        fwd, _ = _lib.model_forward_noisy_wide(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, H.flat(m), nz.params(),
                                               row0=row0, ham_diag=_diag(m))
        torch.cuda.synchronize()
        gap = np.abs(pred - fwd.cpu().numpy()).max()
        print(f'n={n} {kind} {readout} T={T}: max|pred - forward| = {gap:.2e}')
        assert gap <= 1e-13


@pytest.mark.parametrize('n,kind,readout', [(10, 'heaqnn', 'Z'), (11, 'quanonet', 'Y'), (12, 'heaqnn', 'diag')])
def test_a_row_does_not_depend_on_its_batch(dev, n, kind, readout):
    m = build(kind, n, True, readout, seed=4).to(dev)
    rows, cut, base = 7, 3, BIG - 2
    ins, y0 = _on(dev, inputs(kind, rows, seed=8), np.zeros(rows))
    nz = noise_model((0.05, 0.1, 0.05), T=TILE + 3, seed=5)
    g_all, pred = _call(m, ins, y0, nz, row0=base)
    # 7 rows in one call and as 3 + 4 with matching row0: pred bitwise
    _, pa = _call(m, tuple(t[:cut] for t in ins), y0[:cut], nz, row0=base)
    _, pb = _call(m, tuple(t[cut:] for t in ins), y0[cut:], nz, row0=base + cut)
    assert np.array_equal(np.concatenate([pa, pb]), pred)
    g2, p2 = _call(m, ins, y0, nz, row0=base)
    assert np.array_equal(g2, g_all) and np.array_equal(p2, pred)              # and a second call: bitwise
    # One row's contribution, alone: with y = pred everywhere but at row r every other row's weight 2 (pred - y) inv is an
    # exact zero, so grad[:P] is row r's record times its weight -- in the whole batch, in its part of the split, and as a
    # batch of one with its own row0.
    for r in (1, 6):
        y = torch.tensor(pred, device=dev)
        y[r] += 1.0
        whole, _ = _call(m, ins, y, nz, row0=base, inv=0.5)
        lo, hi = (0, cut) if r < cut else (cut, rows)
        part, _ = _call(m, tuple(t[lo:hi] for t in ins), y[lo:hi], nz, row0=base + lo, inv=0.5)
        alone, _ = _call(m, tuple(t[r:r + 1] for t in ins), y[r:r + 1], nz, row0=base + r, inv=0.5)
        assert np.array_equal(whole[:-2], part[:-2]) and np.array_equal(whole[:-2], alone[:-2]), r
        assert np.abs(whole[:-2]).max() > 1e-3


@pytest.mark.parametrize('n,kind,readout,trainable', [(10, 'quanonet', 'Z', True), (11, 'heaqnn', 'diag', True),
                                                      (12, 'quanonet', 'X', False)])
def test_train_steps(dev, n, kind, readout, trainable):
    from quanonet_amd import _lib
    m = build(kind, n, trainable, readout, seed=5).to(dev)
    bounds, sizes = [0, 3, 7, 9], [3, 4, 2]
    ins, y = _on(dev, inputs(kind, bounds[-1], seed=6), np.random.default_rng(6).normal(scale=0.7, size=bounds[-1]))
    desc, diag = m.fused_desc(), _diag(m)
    trunk = ins[1] if len(ins) > 1 else None
    base = noise_model((0.05, 0.1, 0.05), T=TILE + 1, seed=2 ** 64 - 3)          # seed + count wraps mod 2^64
    lr, b1, b2, eps, wd = 3e-2, 0.9, 0.999, 1e-8, 0.0
    P = H.flat(m).numel()
    firsts = {}
    for first in (1, 5):
        p1, m1, v1 = _adam_state(H.flat(m))
        out1 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
        _lib.model_train_steps_noisy_lds(desc, bounds, sizes, ins[0], trunk, y, p1, out1, m1, v1, first, lr, b1, b2, eps, wd,
                                         base.params(), ham_diag=diag)
        # the loop of single calls under seed + count, row0 = the step's first row, then the Adam launch
        p2, m2, v2 = _adam_state(H.flat(m))
        out2 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
        for i in range(3):
            a, b = bounds[i], bounds[i + 1]
            nz = noise_model((0.05, 0.1, 0.05), T=TILE + 1, seed=(base.seed + first + i) % 2 ** 64)
            _lib.model_loss_grad_noisy_lds(desc, ins[0][a:b], None if trunk is None else trunk[a:b], y[a:b], p2, nz.params(),
                                           1.0 / sizes[i], out2[i], row0=a, ham_diag=diag)
            _lib.adam_step(p2, out2[i], m2, v2, first + i, lr, b1, b2, eps, wd)
        torch.cuda.synchronize()
        assert torch.equal(out1, out2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2), first
        assert not torch.equal(p1, H.flat(m))
        firsts[first] = out1[0].cpu().numpy()
    # fresh noise per Adam count: the first step's gradient differs between first_step = 1 and 5 (same parameters, same rows)
    assert not np.array_equal(firsts[1][:P], firsts[5][:P])
    assert firsts[1][P + 1] == firsts[5][P + 1]


def test_refusals_leave_the_outputs_untouched(dev):
    from quanonet_amd import _lib
    m = build('quanonet', 10, True, 'Z').to(dev)
    ins, y = _on(dev, inputs('quanonet', 10), np.random.default_rng(0).normal(size=10))
    desc, params = m.fused_desc(), H.flat(m)
    P = params.numel()
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 20, 1)
    state = lambda: (torch.full((P + 2,), 123.0, dtype=torch.float64, device=dev), torch.full((10,), 456.0, dtype=torch.float64, device=dev),
                     params.clone(), torch.full((P,), 7.0, dtype=torch.float64, device=dev), torch.full((P,), 8.0, dtype=torch.float64, device=dev),
                     torch.full((2, P + 2), 123.0, dtype=torch.float64, device=dev))

    def untouched(st):
        torch.cuda.synchronize()
        g, pr, p, mm, vv, out = st
        return bool(torch.all(g == 123.0) and torch.all(pr == 456.0) and torch.equal(p, params) and torch.all(mm == 7.0)
                    and torch.all(vv == 8.0) and torch.all(out == 123.0))

    def both(d, i, exc, nz, first_step=1, trunk='given'):
        st = state()
        g, pr, p, mm, vv, out = st
        tr = (i[1] if len(i) > 1 else None) if trunk == 'given' else None
        if first_step >= 1:
            with pytest.raises(exc):
                _lib.model_loss_grad_noisy_lds(d, i[0], tr, y, p, nz, 0.1, g, pred=pr)
        with pytest.raises(exc):
            _lib.model_train_steps_noisy_lds(d, [0, 4, 10], [4, 6], i[0], tr, y, p, out, mm, vv, first_step, 1e-2, 0.9, 0.999,
                                             1e-8, 0.0, nz)
        assert untouched(st)

    for bad in (_lib.NoiseParams(-0.01, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.5, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
                _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0), _lib.NoiseParams(0.01, 0.02, 0.03, 100, 20, 1),      # shots > 0
                _lib.NoiseParams(0.01, 0.02, 0.03, 0, 0, 1)):                                                       # trajectories < 1
        both(desc, ins, _lib.QheaError, bad)
    both(desc, ins, _lib.QheaError, ok, trunk=None)                               # a QuanONet without its trunk input
    both(desc, ins, _lib.QheaError, ok, first_step=0)
    for n in (6, 9):                                                              # the exact calls' sizes, and the _wide pair's
        mn = build('heaqnn', n, True, 'Z').to(dev)
        xn, pn = torch.tensor(inputs('heaqnn', 10)[0], device=dev), H.flat(mn)
        gn, prn = torch.full((pn.numel() + 2,), 123.0, dtype=torch.float64, device=dev), torch.full((10,), 456.0, dtype=torch.float64, device=dev)
        mmn, vvn, outn = torch.full_like(pn, 7.0), torch.full_like(pn, 8.0), torch.full((2, pn.numel() + 2), 123.0, dtype=torch.float64, device=dev)
        with pytest.raises(_lib.Unsupported):
            _lib.model_loss_grad_noisy_lds(mn.fused_desc(), xn, None, y, pn, ok, 0.1, gn, pred=prn)
        with pytest.raises(_lib.Unsupported):
            _lib.model_train_steps_noisy_lds(mn.fused_desc(), [0, 4, 10], [4, 6], xn, None, y, pn, outn, mmn, vvn, 1, 1e-2, 0.9,
                                             0.999, 1e-8, 0.0, ok)
        torch.cuda.synchronize()
        assert torch.all(gn == 123.0) and torch.all(prn == 456.0) and torch.all(outn == 123.0) and torch.equal(pn, H.flat(mn))
        assert torch.all(mmn == 7.0) and torch.all(vvn == 8.0)
    # a workspace one byte short and a NULL workspace, through the C ABI itself
    lib = _lib.load()
    need = lib.qhea_model_noisy_lds_grad_workspace_bytes(ctypes.byref(desc), 10, ctypes.byref(ok))
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    st = state()
    g, pr, p, mm, vv, out = st
    ptr = _lib._ptr
    with torch.cuda.device(dev):
        args = (ctypes.byref(desc), 0, 10, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(p), None, ctypes.byref(ok), 0.1, ptr(g), ptr(pr))
        assert lib.qhea_model_loss_grad_noisy_lds(*args, ptr(ws), need - 1, _lib._stream(dev)) == -3
        assert lib.qhea_model_loss_grad_noisy_lds(*args, None, 0, _lib._stream(dev)) == -3
        rb, ib = (ctypes.c_int64 * 3)(0, 4, 10), (ctypes.c_double * 2)(0.25, 1.0 / 6)
        targs = (ctypes.byref(desc), 2, rb, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(p), None, ctypes.byref(ok), ib, ptr(out), P + 2,
                 ptr(mm), ptr(vv), 1, 1e-2, 0.9, 0.999, 1e-8, 0.0)
        # the workspace must fit the largest step (6 rows): the size for 4 rows is refused
        small = lib.qhea_model_noisy_lds_grad_workspace_bytes(ctypes.byref(desc), 4, ctypes.byref(ok))
        assert lib.qhea_model_train_steps_noisy_lds(*targs, ptr(ws), small, _lib._stream(dev)) == -3
        assert lib.qhea_model_train_steps_noisy_lds(*targs, None, 0, _lib._stream(dev)) == -3
        assert untouched(st)
        # an empty batch and an empty schedule are fine and launch nothing
        assert lib.qhea_model_loss_grad_noisy_lds(ctypes.byref(desc), 0, 0, None, None, None, None, None, ctypes.byref(ok), 0.1,
                                                  None, None, None, 0, _lib._stream(dev)) == 0
        assert lib.qhea_model_train_steps_noisy_lds(*((targs[0], 0) + targs[2:]), None, 0, _lib._stream(dev)) == 0
    assert untouched(st)


def _capture_equals_eager(dev, run, fresh, want):
    eager = fresh()
    run(eager)                                                                     # also sizes the workspace outside the capture
    torch.cuda.synchronize()
    scratch = fresh()
    names = [k[0] for k in H.kernel_launches(dev, lambda: run(scratch))]
    assert len(names) == len(want), names
    for got, kernel in zip(names, want):
        assert kernel in got, names
    # the captured call, replayed on fresh state, gives the eager result bitwise
    st = fresh()
    s = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run(st)
    for t, src in zip(st, fresh()):
        t.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(st, eager):
        assert torch.equal(a, b)
    return eager


STEP = ['prep_model_kernel', 'noisy_grad_lds_kernel', 'noisy_grad_fold_kernel', 'reduce_density_kernel']


@pytest.mark.parametrize('readout', ['Z', 'diag'])
def test_graph_capture_and_launch_order(dev, readout):
    """per step: the prep kernel, the trajectory kernel, the fold kernel, the reduce kernel -- and with ham_diag the kernel that
    builds diag' in front, once per call (include/quanonet_hea.h); the single call and two steps of train_steps, each captured
    on one stream"""
    from quanonet_amd import _lib
    m = build('heaqnn', 10, True, readout, seed=1).to(dev)
    ins, y = _on(dev, inputs('heaqnn', 9), np.random.default_rng(2).normal(size=9))
    desc, nz, diag = m.fused_desc(), noise_model((0.05, 0.1, 0.05), T=TILE + 1, seed=8).params(), _diag(m)
    P = H.flat(m).numel()
    mix = ['readout_mix_kernel'] if readout == 'diag' else []
    flat = H.flat(m)

    def single(st):
        grad, pred = st
        _lib.model_loss_grad_noisy_lds(desc, ins[0], None, y, flat, nz, 1.0 / 9, grad, row0=3, ham_diag=diag, pred=pred)

    _capture_equals_eager(dev, single, lambda: (torch.zeros(P + 2, dtype=torch.float64, device=dev),
                                                torch.zeros(9, dtype=torch.float64, device=dev)), mix + STEP)

    def steps(st):
        p, mm, vv, out = st
        _lib.model_train_steps_noisy_lds(desc, [0, 5, 9], [5, 4], ins[0], None, y, p, out, mm, vv, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0,
                                         nz, ham_diag=diag)

    eager = _capture_equals_eager(dev, steps, lambda: (*_adam_state(H.flat(m)), torch.zeros(2, P + 2, dtype=torch.float64, device=dev)),
                                  mix + STEP + STEP)
    assert not torch.equal(eager[0], H.flat(m))
