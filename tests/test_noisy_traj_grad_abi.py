"""
The sampled-trajectory gradient on the GPU (qhea_model_loss_grad_noisy_wide / qhea_model_train_steps_noisy_wide, through
quanonet_amd._lib) against the numpy reference tests/noisy_traj_grad_reference.py, which replays the header's random stream:
the whole [P + 2] buffer and pred at n = 7, 8, 9, noiseless = the ideal call, pred = the forward call's, independence of the
batch, unbiasedness against the CPU density matrix, train_steps = the loop of single calls, refusals, graph capture.
Tolerance against the reference: atol 1e-10, the one the HIP path is held to against the oracle.
Shapes: two blocks per net, sub-layers per block 1 and 2 (tests/test_noisy_traj_grad_reference.py build); the kernel's tile is
4 trajectories, so T = 1, 4 and 5 are one short tile, one full tile, and a full tile followed by a tile of one.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import noisy_traj_grad_reference as TG
from tests.test_noisy_traj_grad_reference import UNBIASED, build, inputs, noise_model, unbiased_case, within_sigmas

pytestmark = pytest.mark.gpu
ATOL = 1e-10
TILE = 4
MID, ALL = (0.05, 0.1), (1.0, 1.0)          # almost every segment draws an error / every location fires
BIG = 3_000_000_000                         # a global row index whose high counter word is in use


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _diag(m):
    q = m.quantum_layer
    return q.ham_diag if q.use_full_ham else None


def _on(dev, ins, y):
    return tuple(torch.tensor(t, device=dev) for t in ins), torch.tensor(np.asarray(y, np.float64), device=dev)


def _call(m, ins, y, nz, row0=0, inv=None, want_pred=True):
    """(grad[P+2], pred[B]) of one qhea_model_loss_grad_noisy_wide call as numpy arrays; m, ins, y on the device"""
    from quanonet_amd import _lib
    flat = H.flat(m)
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device) if want_pred else None
    _lib.model_loss_grad_noisy_wide(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat, nz.params(),
                                    1.0 / rows if inv is None else inv, grad, row0=row0, ham_diag=_diag(m), pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (pred.cpu().numpy() if want_pred else None)


# every value of every axis at each n: model, frequency kind, read-out, readout rate, row0, T, rates
CASES = [('quanonet', True, 'Z', 0.05, 0, TILE + 1, MID),
         ('heaqnn', False, 'X', 0.0, BIG, TILE, ALL),
         ('quanonet', False, 'Y', 0.05, BIG, 1, MID),
         ('heaqnn', True, 'diag', 0.05, 0, TILE + 1, ALL),
         ('heaqnn', True, 'diag', 0.0, BIG, TILE, MID)]


@pytest.mark.parametrize('n', [7, 8, 9])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_against_the_reference(dev, n, case):
    kind, trainable, readout, q, row0, T, (p1, p2) = CASES[case]
    rows = 5                                                  # not a multiple of the four waves of a workgroup
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


@pytest.mark.parametrize('n', [7, 8, 9])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_noiseless_equals_ideal(dev, n, kind):
    from quanonet_amd import _lib
    for trainable, readout in ((True, 'Z'), (False, 'X'), (True, 'Y'), (False, 'diag')):
        m = build(kind, n, trainable, readout, seed=n).to(dev)
        rows = 37
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


@pytest.mark.parametrize('n,kind,readout', [(7, 'quanonet', 'Z'), (8, 'heaqnn', 'diag'), (9, 'quanonet', 'X'), (8, 'heaqnn', 'Y')])
def test_pred_is_the_forward_calls(dev, n, kind, readout):
    """same noise and row0: the two calls add the same trajectory values in different tiles; the bound is the one the exact
    gradient call's pred is held to against its forward call (1e-13)"""
    from quanonet_amd import _lib
    m = build(kind, n, True, readout, seed=n).to(dev)
    rows = 23
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


@pytest.mark.parametrize('n,kind,readout', [(7, 'heaqnn', 'Z'), (8, 'quanonet', 'Y'), (9, 'heaqnn', 'diag')])
def test_a_row_does_not_depend_on_its_batch(dev, n, kind, readout):
    cpu, m = build(kind, n, True, readout, seed=4), build(kind, n, True, readout, seed=4).to(dev)
    rows, cut, base = 11, 4, BIG - 3
    ins, y0 = _on(dev, inputs(kind, rows, seed=8), np.zeros(rows))
    nz = noise_model((0.05, 0.1, 0.05), T=TILE + 3, seed=5)
    g_all, pred = _call(m, ins, y0, nz, row0=base)
    # 11 rows in one call and as 4 + 7 with matching row0: pred bitwise
    _, pa = _call(m, tuple(t[:cut] for t in ins), y0[:cut], nz, row0=base)
    _, pb = _call(m, tuple(t[cut:] for t in ins), y0[cut:], nz, row0=base + cut)
    assert np.array_equal(np.concatenate([pa, pb]), pred)
    g2, p2 = _call(m, ins, y0, nz, row0=base)
    assert np.array_equal(g2, g_all) and np.array_equal(p2, pred)              # and a second call: bitwise
    # One row's contribution, alone: with y = pred everywhere but at row r every other row's weight 2 (pred - y) inv is an
    # exact zero, so grad[:P] is row r's record times its weight -- in the whole batch, in its part of the split, and as a
    # batch of one with its own row0.
    for r in (1, 6, 10):
        y = torch.tensor(pred, device=dev)
        y[r] += 1.0
        whole, _ = _call(m, ins, y, nz, row0=base, inv=0.5)
        lo, hi = (0, cut) if r < cut else (cut, rows)
        part, _ = _call(m, tuple(t[lo:hi] for t in ins), y[lo:hi], nz, row0=base + lo, inv=0.5)
        alone, _ = _call(m, tuple(t[r:r + 1] for t in ins), y[r:r + 1], nz, row0=base + r, inv=0.5)
        assert np.array_equal(whole[:-2], part[:-2]) and np.array_equal(whole[:-2], alone[:-2]), r
        assert np.abs(whole[:-2]).max() > 1e-3
        # grad(y) - grad(y + 1) of the batch of one is the row's d pred / d params: the reference's
        other, _ = _call(m, tuple(t[r:r + 1] for t in ins), y[r:r + 1] + 1.0, nz, row0=base + r, inv=0.5)
        ref = TG.dpred(cpu, tuple(t[r:r + 1].cpu().numpy() for t in ins), TG.TrajEngine(nz, base + r))
        np.testing.assert_allclose((alone - other)[:-2], ref, rtol=0, atol=ATOL)


def test_unbiasedness(dev):
    """K seeds of T trajectories: every component of the mean of d pred / d params lies within 5 standard errors (across the
    seeds) of the exact noisy derivative of the CPU density matrix.  tests/test_noisy_traj_grad_reference.py checks the same
    condition, seeds and T on the reference alone; the GPU equals the reference to 1e-10, so this is deterministic."""
    u = UNBIASED
    cpu, ins_np = unbiased_case()
    exact = TG.dpred(cpu, ins_np, TG.ExactEngine(noise_model(u['rates'])))
    m = cpu.to(dev)
    ins, y0 = _on(dev, ins_np, np.zeros(1))
    per_seed = []
    for s in u['seeds']:
        nz = noise_model(u['rates'], T=u['T'], seed=s)
        g0, _ = _call(m, ins, y0, nz, inv=0.5, want_pred=False)
        g1, _ = _call(m, ins, y0 + 1.0, nz, inv=0.5, want_pred=False)
        per_seed.append((g0 - g1)[:-2])
    ok, worst = within_sigmas(per_seed, exact, u['sigmas'])
    print(f"K={u['K']} T={u['T']}: worst deviation {worst:.2f} standard errors over {exact.size} components")
    assert exact.size == sum(p.numel() for p in m.parameters())                # no component left out
    assert ok, worst


def _adam_state(flat):
    return flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)


@pytest.mark.parametrize('n,kind,readout,trainable', [(7, 'quanonet', 'Z', True), (8, 'heaqnn', 'diag', True),
                                                      (9, 'quanonet', 'X', False)])
def test_train_steps(dev, n, kind, readout, trainable):
    from quanonet_amd import _lib
    m = build(kind, n, trainable, readout, seed=5).to(dev)
    bounds, sizes = [0, 5, 12, 15], [5, 7, 3]
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
        _lib.model_train_steps_noisy_wide(desc, bounds, sizes, ins[0], trunk, y, p1, out1, m1, v1, first, lr, b1, b2, eps, wd,
                                          base.params(), ham_diag=diag)
        # the loop of single calls under seed + count, row0 = the step's first row, then the Adam launch
        p2, m2, v2 = _adam_state(H.flat(m))
        out2 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
        for i in range(3):
            a, b = bounds[i], bounds[i + 1]
            nz = noise_model((0.05, 0.1, 0.05), T=TILE + 1, seed=(base.seed + first + i) % 2 ** 64)
            _lib.model_loss_grad_noisy_wide(desc, ins[0][a:b], None if trunk is None else trunk[a:b], y[a:b], p2, nz.params(),
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
    m = build('quanonet', 7, True, 'Z').to(dev)
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
                _lib.model_loss_grad_noisy_wide(d, i[0], tr, y, p, nz, 0.1, g, pred=pr)
        with pytest.raises(exc):
            _lib.model_train_steps_noisy_wide(d, [0, 4, 10], [4, 6], i[0], tr, y, p, out, mm, vv, first_step, 1e-2, 0.9, 0.999,
                                              1e-8, 0.0, nz)
        assert untouched(st)

    for bad in (_lib.NoiseParams(-0.01, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.5, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
                _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0), _lib.NoiseParams(0.01, 0.02, 0.03, 100, 20, 1),      # shots > 0
                _lib.NoiseParams(0.01, 0.02, 0.03, 0, 0, 1)):                                                       # trajectories < 1
        both(desc, ins, _lib.QheaError, bad)
    both(desc, ins, _lib.QheaError, ok, trunk=None)                               # a QuanONet without its trunk input
    both(desc, ins, _lib.QheaError, ok, first_step=0)
    for n in (6, 10):                                                             # the exact calls' sizes, and the LDS sizes
        mn = build('heaqnn', n, True, 'Z').to(dev)
        xn, pn = torch.tensor(inputs('heaqnn', 10)[0], device=dev), H.flat(mn)
        gn, prn = torch.full((pn.numel() + 2,), 123.0, dtype=torch.float64, device=dev), torch.full((10,), 456.0, dtype=torch.float64, device=dev)
        mmn, vvn, outn = torch.full_like(pn, 7.0), torch.full_like(pn, 8.0), torch.full((2, pn.numel() + 2), 123.0, dtype=torch.float64, device=dev)
        with pytest.raises(_lib.Unsupported):
            _lib.model_loss_grad_noisy_wide(mn.fused_desc(), xn, None, y, pn, ok, 0.1, gn, pred=prn)
        with pytest.raises(_lib.Unsupported):
            _lib.model_train_steps_noisy_wide(mn.fused_desc(), [0, 4, 10], [4, 6], xn, None, y, pn, outn, mmn, vvn, 1, 1e-2, 0.9,
                                              0.999, 1e-8, 0.0, ok)
        torch.cuda.synchronize()
        assert torch.all(gn == 123.0) and torch.all(prn == 456.0) and torch.all(outn == 123.0) and torch.equal(pn, H.flat(mn))
        assert torch.all(mmn == 7.0) and torch.all(vvn == 8.0)
    # a workspace one byte short, through the C ABI itself
    lib = _lib.load()
    need = lib.qhea_model_noisy_wide_grad_workspace_bytes(ctypes.byref(desc), 10, ctypes.byref(ok))
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    st = state()
    g, pr, p, mm, vv, out = st
    ptr = _lib._ptr
    with torch.cuda.device(dev):
        args = (ctypes.byref(desc), 0, 10, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(p), None, ctypes.byref(ok), 0.1, ptr(g), ptr(pr))
        assert lib.qhea_model_loss_grad_noisy_wide(*args, ptr(ws), need - 1, _lib._stream(dev)) == -3
        assert lib.qhea_model_loss_grad_noisy_wide(*args, None, 0, _lib._stream(dev)) == -3
        rb, ib = (ctypes.c_int64 * 3)(0, 4, 10), (ctypes.c_double * 2)(0.25, 1.0 / 6)
        targs = (ctypes.byref(desc), 2, rb, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(p), None, ctypes.byref(ok), ib, ptr(out), P + 2,
                 ptr(mm), ptr(vv), 1, 1e-2, 0.9, 0.999, 1e-8, 0.0)
        # the workspace must fit the largest step (6 rows): the size for 4 rows is refused
        small = lib.qhea_model_noisy_wide_grad_workspace_bytes(ctypes.byref(desc), 4, ctypes.byref(ok))
        assert lib.qhea_model_train_steps_noisy_wide(*targs, ptr(ws), small, _lib._stream(dev)) == -3
        assert untouched(st)
        # an empty batch and an empty schedule are fine and launch nothing
        assert lib.qhea_model_loss_grad_noisy_wide(ctypes.byref(desc), 0, 0, None, None, None, None, None, ctypes.byref(ok), 0.1,
                                                   None, None, None, 0, _lib._stream(dev)) == 0
        assert lib.qhea_model_train_steps_noisy_wide(*((targs[0], 0) + targs[2:]), None, 0, _lib._stream(dev)) == 0
    assert untouched(st)


@pytest.mark.parametrize('readout,launches', [('Z', 4), ('diag', 5)])
def test_graph_capture_and_launch_count(dev, readout, launches):
    """one step: the prep kernel, the trajectory kernel, the fold kernel, the reduce kernel -- and with ham_diag the kernel that
    builds diag' in front, once per call (include/quanonet_hea.h)"""
    from quanonet_amd import _lib
    m = build('heaqnn', 8, True, readout, seed=1).to(dev)
    bounds, sizes = [0, 9], [9]
    ins, y = _on(dev, inputs('heaqnn', 9), np.random.default_rng(2).normal(size=9))
    desc, nz, diag = m.fused_desc(), noise_model((0.05, 0.1, 0.05), T=TILE + 1, seed=8).params(), _diag(m)
    P = H.flat(m).numel()

    def run(st):
        p, mm, vv, out = st
        _lib.model_train_steps_noisy_wide(desc, bounds, sizes, ins[0], None, y, p, out, mm, vv, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0, nz,
                                          ham_diag=diag)

    fresh = lambda: (*_adam_state(H.flat(m)), torch.zeros(1, P + 2, dtype=torch.float64, device=dev))
    eager = fresh()
    run(eager)                                                                     # also sizes the workspace outside the capture
    torch.cuda.synchronize()
    scratch = fresh()
    names = [k[0] for k in H.kernel_launches(dev, lambda: run(scratch))]
    want = (['readout_mix_kernel'] if readout == 'diag' else []) + ['prep_model_kernel', 'noisy_grad_wave_kernel',
                                                                    'noisy_grad_fold_kernel', 'reduce_density_kernel']
    assert len(names) == launches == len(want), names
    for got, kernel in zip(names, want):
        assert kernel in got, names
    # the captured step, replayed on fresh state, gives the eager result bitwise
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
    assert not torch.equal(eager[0], H.flat(m))
