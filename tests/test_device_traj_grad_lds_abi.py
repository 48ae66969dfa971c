"""
The quantum-jump trajectory gradient at n = 10..12 on the GPU (qhea_model_loss_grad_noisy_device_lds /
qhea_model_train_steps_noisy_device_lds, through quanonet_amd._lib, quanonet_amd.noise.device_trajectory_loss_and_grad and the
solver key train_jump_trajectories) against the numpy reference tests/device_traj_grad_reference.py, which replays the header's
random stream with the kernel's unnormalised rule: the whole [P + 2] buffer and pred at n = 10, 11, 12 under the five cases of
tests/test_device_traj_grad_abi.py, the 2^100 rescale, all rates zero = the ideal call, pred = the forward call's, independence
of batch, grid and chunking, train_steps = the loop of single calls, graph capture, refusals, and the Python layers.

Tolerance against the reference: atol 1e-10, the project's bound for this family.  A jump decision u N2 < gamma M differs between
kernel and numpy only where u lies within a few ulps (1e-15 relative) of the edge: the cases here make fewer than 1e5 decisions,
a chance below 1e-10 over the set -- the argument of tests/test_device_traj_grad_abi.py.  No row is excluded.
Shapes: two blocks per net, sub-layers per block 1 and 2; the kernel's tile is 2 trajectories, so T = 1, 2 and 3 (the n = 7..9
cases' 1, 4, 5) are one short tile, one full tile, and a full tile followed by a tile of one.  Every n runs four gate qubits per
pass (a ragged last pass at n = 10 and 11).
No unbiasedness check here: the exact derivative would need a 4^10-entry density matrix on the CPU.  The estimator is the one
tests/test_device_traj_grad_abi.py and tests/test_device_traj_grad_reference.py check at n = 7 and 2; what is new is the walk,
which the reference comparison pins.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import device_traj_grad_reference as G
from tests import helpers as H
from tests import noisy_traj_grad_reference as TG
from tests.test_device_traj_grad_abi import BIG, CASES, _adam_state, _cfg, _diag, _on, _run, as_dict, quiet, setting
from tests.test_noisy_forward import _circuit, _solver_data
from tests.test_noisy_traj_grad_reference import build, inputs

pytestmark = pytest.mark.gpu
ATOL = 1e-10
NS = [10, 11, 12]
TILE = 2
TMAP = {1: 1, 4: TILE, 5: TILE + 1}
JUMPY = [c for c in range(len(CASES)) if CASES[c][3] in ('strong', 'polar')]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _call(m, ins, y, dn, sp, row0=0, inv=None, want_pred=True):
    """(grad[P+2], pred[B]) of one qhea_model_loss_grad_noisy_device_lds call as numpy arrays; m, ins, y on the device"""
    from quanonet_amd import _lib
    flat = H.flat(m)
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device) if want_pred else None
    _lib.model_loss_grad_noisy_device_lds(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat,
                                          dn.params(m.num_qubits), sp.params(), 1.0 / rows if inv is None else inv, grad, row0=row0,
                                          ham_diag=_diag(m), pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (pred.cpu().numpy() if want_pred else None)


def _case(n, case):
    from quanonet_amd.noise import Sampling
    kind, trainable, readout, what, idle, asym, row0, T = CASES[case]
    rows = 3
    cpu = build(kind, n, trainable, readout, seed=n + case, net=(2, 1) if case == 4 else None)
    ins, y = inputs(kind, rows, seed=case), np.random.default_rng(n + case).normal(scale=0.7, size=rows)
    dn, sp = setting(what, n, idle, asym, seed=case), Sampling(trajectories=TMAP[T], seed=1234 + case)
    return cpu, ins, y, dn, sp, row0, rows


@functools.lru_cache(maxsize=None)
def _coverage(n, case):
    """what the replay of a case covers: computed once per (n, case), shared by the comparison and the per-n union"""
    cpu, ins, _, dn, sp, row0, rows = _case(n, case)
    c, _ = _circuit(cpu, tuple(torch.as_tensor(t) for t in ins))
    r = G.walk(c['n'], c['cfgs'], c['x'], c['w'], as_dict(dn, n), sp.trajectories, sp.seed, c['offset'], c['coeff'], c['ham_diag'],
               c['ham_pauli'], row0=row0, grad=False)
    M = r['N2'].shape[0]
    jumps = np.zeros(M, dtype=np.int64)
    per_seg, groups = {}, [0, 0, 0]
    first_enc = last_ctl = last_tgt = polar = 0
    for fire, (blk, seg, kind, q, slot), pol in zip(r['pattern'], r['sites'], r['polarity']):
        jumps += fire
        per_seg[seg] = per_seg.get(seg, 0) + fire.astype(np.int64)
        groups[min(q // 4, 2)] += int(fire.sum())
        first_enc += int(fire.sum()) if kind == G.ENC and q == 0 else 0
        last_ctl += int(fire.sum()) if kind == G.CTL and slot == n - 1 else 0
        last_tgt += int(fire.sum()) if kind == G.TGT and slot == n - 1 else 0
        polar += int((fire & pol).sum())
    most = np.max(np.stack(list(per_seg.values())), axis=0) if per_seg else np.zeros(M, dtype=np.int64)
    return {'jumps': jumps, 'most_in_segment': most, 'groups': groups, 'first_enc': first_enc, 'last_ctl': last_ctl,
            'last_tgt': last_tgt, 'polarity': polar, 'dephasing': r['counts']['dephasing'], 'pauli': r['counts']['pauli'],
            'decisions': len(r['sites']) * M}


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('case', range(len(CASES)))
def test_against_the_reference(dev, n, case):
    kind, trainable, readout, what, idle, asym, _, _ = CASES[case]
    cpu, ins, y, dn, sp, row0, rows = _case(n, case)
    T = sp.trajectories
    # what the case is about happens in the compared rows, or it shows nothing
    cov = _coverage(n, case)
    assert cov['decisions'] < 1e5
    if what == 'none':
        assert cov['jumps'].size == rows * T and cov['jumps'].sum() == 0 and cov['dephasing'] == 0 and cov['pauli'] >= 1, cov
    elif what == 'dephasing':
        assert cov['jumps'].sum() == 0 and cov['dephasing'] >= rows * T, cov
    else:
        assert cov['jumps'].min() >= 2 and cov['most_in_segment'].max() >= 2, cov      # re-walks, and a re-entered pass
        assert min(cov['groups']) >= 1 and cov['polarity'] >= 1, cov                    # every pass's wires; a flipped site
    ref, ref_pred = TG.model_loss_grad(cpu, ins, y, 1.0 / 7, G.DeviceTrajEngine(as_dict(dn, n), T, sp.seed, row0))
    grad, pred = _call(cpu.to(dev), *_on(dev, ins, y), dn, sp, row0=row0, inv=1.0 / 7)
    tag = f'n={n} {kind} trainable={trainable} {readout} {what} idle={idle} asym={asym} row0={row0} T={T}'
    print(f'{tag}: max|grad err|={np.abs(grad - ref).max():.2e} max|pred err|={np.abs(pred - ref_pred).max():.2e} '
          f'max|grad|={np.abs(ref[:-2]).max():.2e} jumps={cov["jumps"].min()}..{cov["jumps"].max()} '
          f'most in a segment={int(cov["most_in_segment"].max())} polarity={cov["polarity"]}')
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL, err_msg=tag)


@pytest.mark.parametrize('n', NS)
def test_the_cases_cover_the_special_sites(n):
    """over the strong and polar cases of an n, which test_against_the_reference compares: a jump at a block's first encoding
    site, at the ring's last CTL site, and at the TGT site behind slot n - 1 (the three-bit mask)"""
    covs = [_coverage(n, c) for c in JUMPY]
    assert len(covs) == 3
    for key in ('first_enc', 'last_ctl', 'last_tgt'):
        assert sum(c[key] for c in covs) >= 1, (n, key, [c[key] for c in covs])


def test_the_rescale_on_the_gpu(dev):
    """one block of 31 segments under gamma = 1 - exp(-7): both trajectories fire 135 and more jumps and the 2^-200 rescale; the
    walk crosses it both ways, and these are the longest re-walks a test runs"""
    from quanonet_amd.noise import DeviceNoise, Sampling
    n = 10
    cpu = build('heaqnn', n, True, 'Z', seed=10, net=(1, 30))
    ins, y = inputs('heaqnn', 1, seed=3), np.array([0.3])
    dn, sp = DeviceNoise(p1=0.01, t1=1.0, t2=2.0, t_rx=7.0, t_rot=7.0, t_cx=7.0, idle=False), Sampling(trajectories=2, seed=1)
    c, _ = _circuit(cpu, tuple(torch.as_tensor(t) for t in ins))
    r = G.walk(c['n'], c['cfgs'], c['x'], c['w'], as_dict(dn, n), 2, 1, c['offset'], c['coeff'], c['ham_diag'], c['ham_pauli'],
               grad=False)
    jumps = G.coverage(r, n, 2)['jumps']
    assert r['rescaled'].min() >= 1 and jumps.min() >= 100, (r['rescaled'], jumps)
    ref, ref_pred = TG.model_loss_grad(cpu, ins, y, 1.0, G.DeviceTrajEngine(as_dict(dn, n), 2, 1, 0))
    grad, pred = _call(cpu.to(dev), *_on(dev, ins, y), dn, sp, inv=1.0)
    scale = max(1.0, np.abs(ref).max())
    print(f'jumps {jumps} rescales {r["rescaled"]}: max|grad err|={np.abs(grad - ref).max():.2e} (max|ref|={np.abs(ref).max():.2e}) '
          f'max|pred err|={np.abs(pred - ref_pred).max():.2e}')
    assert np.all(np.isfinite(grad))
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL * scale)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL * scale)


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_all_rates_zero_equals_ideal(dev, n, kind):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise, Sampling
    for trainable, readout in ((True, 'Z'), (False, 'X'), (True, 'Y'), (False, 'diag')):
        m = build(kind, n, trainable, readout, seed=n).to(dev)
        rows = 7
        ins, y = _on(dev, inputs(kind, rows, seed=rows), np.random.default_rng(rows).normal(size=rows))
        grad, pred = _call(m, ins, y, DeviceNoise(), Sampling(trajectories=1, seed=3), row0=11)
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
    """same setting, sampling and row0: the two calls add the same trajectory values in different tiles (1e-13)"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import Sampling
    m = build(kind, n, True, readout, seed=n).to(dev)
    rows = 5
    ins, y = _on(dev, inputs(kind, rows, seed=2), np.zeros(rows))
    dn = setting('strong', n)
    for T, row0 in ((1, 0), (TILE + 1, BIG), (70, 5)):
        sp = Sampling(trajectories=T, seed=77)
        _, pred = _call(m, ins, y, dn, sp, row0=row0)
        fwd, _ = _lib.model_forward_noisy_device_wide(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, H.flat(m),
                                                      dn.params(n), sp.params(), row0=row0, ham_diag=_diag(m))
        torch.cuda.synchronize()
        gap = np.abs(pred - fwd.cpu().numpy()).max()
        print(f'n={n} {kind} {readout} T={T}: max|pred - forward| = {gap:.2e}')
        assert gap <= 1e-13


@pytest.mark.parametrize('n,kind,readout', [(10, 'heaqnn', 'Z'), (11, 'quanonet', 'Y'), (12, 'heaqnn', 'diag')])
def test_a_row_does_not_depend_on_its_batch(dev, n, kind, readout):
    from quanonet_amd.noise import Sampling
    cpu, m = build(kind, n, True, readout, seed=4), build(kind, n, True, readout, seed=4).to(dev)
    rows, cut, base = 7, 3, BIG - 3
    ins, y0 = _on(dev, inputs(kind, rows, seed=8), np.zeros(rows))
    dn, sp = setting('strong', n, seed=2), Sampling(trajectories=TILE + 1, seed=5)
    g_all, pred = _call(m, ins, y0, dn, sp, row0=base)
    _, pa = _call(m, tuple(t[:cut] for t in ins), y0[:cut], dn, sp, row0=base)
    _, pb = _call(m, tuple(t[cut:] for t in ins), y0[cut:], dn, sp, row0=base + cut)
    assert np.array_equal(np.concatenate([pa, pb]), pred)
    g2, p2 = _call(m, ins, y0, dn, sp, row0=base)
    assert np.array_equal(g2, g_all) and np.array_equal(p2, pred)              # and a second call: bitwise
    # one row's record alone (y = pred elsewhere makes every other weight an exact zero): in the whole batch, in its part of
    # the split, and as a batch of one with its own row0
    for r in (1, 6):
        y = torch.tensor(pred, device=dev)
        y[r] += 1.0
        whole, _ = _call(m, ins, y, dn, sp, row0=base, inv=0.5)
        lo, hi = (0, cut) if r < cut else (cut, rows)
        part, _ = _call(m, tuple(t[lo:hi] for t in ins), y[lo:hi], dn, sp, row0=base + lo, inv=0.5)
        alone, _ = _call(m, tuple(t[r:r + 1] for t in ins), y[r:r + 1], dn, sp, row0=base + r, inv=0.5)
        assert np.array_equal(whole[:-2], part[:-2]) and np.array_equal(whole[:-2], alone[:-2]), r
        assert np.abs(whole[:-2]).max() > 1e-3


def test_more_items_than_workgroups(dev):
    """more (row, tile) items than qhea_noisy_device_lds_grad_max_workgroups(10): the grid-stride loop takes a second round, and
    the rows are bitwise what they are when called in chunks"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import Sampling
    cap = _lib.noisy_device_lds_grad_max_workgroups(10)
    T = 2 * TILE                                                                  # two items per row
    rows = cap // 2 + 38
    assert cap > 0 and rows * 2 > cap
    m = build('heaqnn', 10, True, 'Z', seed=1, net=(1, 1)).to(dev)
    ins, y0 = _on(dev, inputs('heaqnn', rows, seed=3), np.zeros(rows))
    dn, sp = setting('strong', 10), Sampling(trajectories=T, seed=9)
    _, pred = _call(m, ins, y0, dn, sp, row0=0)
    chunks = [(0, 200), (200, cap // 2), (cap // 2, rows)]
    parts = [_call(m, tuple(t[a:b] for t in ins), y0[a:b], dn, sp, row0=a)[1] for a, b in chunks]
    assert np.array_equal(np.concatenate(parts), pred)
    for r in (0, cap // 2 - 1, rows - 1):                                       # the first round, its last item, the second round
        y = torch.tensor(pred, device=dev)
        y[r] += 1.0
        whole, _ = _call(m, ins, y, dn, sp, inv=0.5)
        alone, _ = _call(m, tuple(t[r:r + 1] for t in ins), y[r:r + 1], dn, sp, row0=r, inv=0.5)
        assert np.array_equal(whole[:-2], alone[:-2]) and np.abs(whole[:-2]).max() > 1e-3, r


@pytest.mark.parametrize('n,kind,readout,trainable', [(10, 'quanonet', 'Z', True), (11, 'heaqnn', 'diag', True),
                                                      (12, 'quanonet', 'X', False)])
def test_train_steps(dev, n, kind, readout, trainable):
    from quanonet_amd import _lib
    from quanonet_amd.noise import Sampling
    m = build(kind, n, trainable, readout, seed=5).to(dev)
    bounds, sizes = [0, 3, 7, 9], [3, 4, 2]
    ins, y = _on(dev, inputs(kind, bounds[-1], seed=6), np.random.default_rng(6).normal(scale=0.7, size=bounds[-1]))
    desc, diag = m.fused_desc(), _diag(m)
    trunk = ins[1] if len(ins) > 1 else None
    dn = setting('strong', n, seed=3)
    base = Sampling(trajectories=TILE + 1, seed=2 ** 64 - 3)                     # seed + count wraps mod 2^64
    lr, b1, b2, eps, wd = 3e-2, 0.9, 0.999, 1e-8, 0.0
    P = H.flat(m).numel()
    firsts = {}
    for first in (1, 5):
        p1, m1, v1 = _adam_state(H.flat(m))
        out1 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
        _lib.model_train_steps_noisy_device_lds(desc, bounds, sizes, ins[0], trunk, y, p1, out1, m1, v1, first, lr, b1, b2, eps, wd,
                                                dn.params(n), base.params(), ham_diag=diag)
        p2, m2, v2 = _adam_state(H.flat(m))
        out2 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
        for i in range(3):
            a, b = bounds[i], bounds[i + 1]
            sp = Sampling(trajectories=TILE + 1, seed=(base.seed + first + i) % 2 ** 64)
            _lib.model_loss_grad_noisy_device_lds(desc, ins[0][a:b], None if trunk is None else trunk[a:b], y[a:b], p2, dn.params(n),
                                                  sp.params(), 1.0 / sizes[i], out2[i], row0=a, ham_diag=diag)
            _lib.adam_step(p2, out2[i], m2, v2, first + i, lr, b1, b2, eps, wd)
        torch.cuda.synchronize()
        assert torch.equal(out1, out2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2), first
        assert not torch.equal(p1, H.flat(m))
        firsts[first] = out1[0].cpu().numpy()
    assert not np.array_equal(firsts[1][:P], firsts[5][:P])                      # fresh draws per Adam count
    assert firsts[1][P + 1] == firsts[5][P + 1]


@pytest.mark.parametrize('readout', ['Z', 'diag'])
def test_graph_capture_and_launch_count(dev, readout):
    """per call the kernel that writes the per-site constants and h', per step the prep kernel, the trajectory kernel, the fold
    kernel and the reduce kernel (include/quanonet_hea.h): the single call and two steps, each captured once and replayed"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import Sampling
    n = 10
    m = build('heaqnn', n, True, readout, seed=1).to(dev)
    bounds, sizes = [0, 4, 9], [4, 5]
    ins, y = _on(dev, inputs('heaqnn', 9), np.random.default_rng(2).normal(size=9))
    desc, diag = m.fused_desc(), _diag(m)
    dn, sp = setting('strong', n).params(n), Sampling(trajectories=TILE + 1, seed=8).params()
    P = H.flat(m).numel()
    step = ['prep_model_kernel', 'device_grad_lds_kernel', 'noisy_grad_fold_kernel', 'reduce_density_kernel']

    def steps(st):
        p, mm, vv, out = st
        _lib.model_train_steps_noisy_device_lds(desc, bounds, sizes, ins[0], None, y, p, out, mm, vv, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0,
                                                dn, sp, ham_diag=diag)

    def single(st):
        p, _, _, out = st
        _lib.model_loss_grad_noisy_device_lds(desc, ins[0], None, y, p, dn, sp, 1.0 / 9, out[0], row0=3, ham_diag=diag)

    fresh = lambda: (*_adam_state(H.flat(m)), torch.zeros(2, P + 2, dtype=torch.float64, device=dev))
    for run, want in ((single, ['device_grad_lds_tables_kernel'] + step), (steps, ['device_grad_lds_tables_kernel'] + 2 * step)):
        eager = fresh()
        run(eager)                                                                 # also sizes the workspace outside the capture
        torch.cuda.synchronize()
        scratch = fresh()
        names = [k[0] for k in H.kernel_launches(dev, lambda: run(scratch))]
        assert len(names) == len(want), names
        for got, kernel in zip(names, want):
            assert kernel in got, names
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
        assert eager[3].abs().sum().item() > 0.0


def test_refusals_leave_the_outputs_untouched(dev):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    from tests.test_device_noise_abi import _record
    n = 10
    m = build('quanonet', n, True, 'Z').to(dev)
    ins, y = _on(dev, inputs('quanonet', 10), np.random.default_rng(0).normal(size=10))
    desc, params = m.fused_desc(), H.flat(m)
    P = params.numel()
    dn, ok = setting('strong', n), _lib.SamplingParams(0, 20, 1)
    state = lambda: (torch.full((P + 2,), 123.0, dtype=torch.float64, device=dev), torch.full((10,), 456.0, dtype=torch.float64, device=dev),
                     params.clone(), torch.full((P,), 7.0, dtype=torch.float64, device=dev), torch.full((P,), 8.0, dtype=torch.float64, device=dev),
                     torch.full((2, P + 2), 123.0, dtype=torch.float64, device=dev))

    def untouched(st):
        torch.cuda.synchronize()
        g, pr, p, mm, vv, out = st
        return bool(torch.all(g == 123.0) and torch.all(pr == 456.0) and torch.equal(p, params) and torch.all(mm == 7.0)
                    and torch.all(vv == 8.0) and torch.all(out == 123.0))

    def both(d, i, exc, rec, sp, first_step=1, trunk='given', match=None):
        st = state()
        g, pr, p, mm, vv, out = st
        tr = (i[1] if len(i) > 1 else None) if trunk == 'given' else None
        if first_step >= 1:
            with pytest.raises(exc, match=match):
                _lib.model_loss_grad_noisy_device_lds(d, i[0], tr, y, p, rec, sp, 0.1, g, pred=pr)
        with pytest.raises(exc, match=match):
            _lib.model_train_steps_noisy_device_lds(d, [0, 4, 10], [4, 6], i[0], tr, y, p, out, mm, vv, first_step, 1e-2, 0.9, 0.999,
                                                    1e-8, 0.0, rec, sp)
        assert untouched(st)

    for bad in (_lib.SamplingParams(1, 20, 1), _lib.SamplingParams(0, 0, 1), _lib.SamplingParams(-1, 20, 1)):
        both(desc, ins, _lib.QheaError, dn.params(n), bad)                        # shots = 1, T = 0
    both(desc, ins, _lib.QheaError, _record(n, p1=[1.5] * n), ok)                 # a bad device record
    both(desc, ins, _lib.QheaError, dn.params(n), ok, trunk=None)                 # a QuanONet without its trunk input
    both(desc, ins, _lib.QheaError, dn.params(n), ok, first_step=0)
    # a site with gamma = 1: named in the message
    dead = DeviceNoise(t1=[1.0] * (n - 1) + [1e-3], t2=[1.0] * (n - 1) + [1e-3], t_rx=0.001, t_rot=0.001, t_cx=0.1, idle=False)
    both(desc, ins, _lib.QheaError, dead.params(n), ok, match=f'CTL on wire {n - 1}')
    m9 = build('heaqnn', 9, True, 'Z').to(dev)
    x9, p9 = torch.tensor(inputs('heaqnn', 10)[0], device=dev), H.flat(m9)
    g9, pr9 = torch.full((p9.numel() + 2,), 123.0, dtype=torch.float64, device=dev), torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    mm9, vv9, out9 = torch.full_like(p9, 7.0), torch.full_like(p9, 8.0), torch.full((2, p9.numel() + 2), 123.0, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.Unsupported, match='10..12'):
        _lib.model_loss_grad_noisy_device_lds(m9.fused_desc(), x9, None, y, p9, setting('strong', 9).params(9), ok, 0.1, g9, pred=pr9)
    with pytest.raises(_lib.Unsupported):
        _lib.model_train_steps_noisy_device_lds(m9.fused_desc(), [0, 4, 10], [4, 6], x9, None, y, p9, out9, mm9, vv9, 1, 1e-2, 0.9,
                                                0.999, 1e-8, 0.0, setting('strong', 9).params(9), ok)
    torch.cuda.synchronize()
    assert torch.all(g9 == 123.0) and torch.all(pr9 == 456.0) and torch.all(out9 == 123.0) and torch.equal(p9, H.flat(m9))
    assert torch.all(mm9 == 7.0) and torch.all(vv9 == 8.0)
    # a NULL sampling and a workspace one byte short, through the C ABI itself
    lib = _lib.load()
    rec = dn.params(n)
    need = lib.qhea_model_noisy_device_lds_grad_workspace_bytes(ctypes.byref(desc), 10, ctypes.byref(ok))
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    st = state()
    g, pr, p, mm, vv, out = st
    ptr = _lib._ptr
    with torch.cuda.device(dev):
        head = (ctypes.byref(desc), 0, 10, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(p), None, ctypes.byref(rec))
        tail = (0.1, ptr(g), ptr(pr))
        call, steps = lib.qhea_model_loss_grad_noisy_device_lds, lib.qhea_model_train_steps_noisy_device_lds
        assert call(*head, None, *tail, ptr(ws), need, _lib._stream(dev)) == -1
        assert call(*head, ctypes.byref(ok), *tail, ptr(ws), need - 1, _lib._stream(dev)) == -3
        assert call(*head, ctypes.byref(ok), *tail, None, 0, _lib._stream(dev)) == -3
        rb, ib = (ctypes.c_int64 * 3)(0, 4, 10), (ctypes.c_double * 2)(0.25, 1.0 / 6)
        targs = (ctypes.byref(desc), 2, rb, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(p), None, ctypes.byref(rec), ctypes.byref(ok), ib,
                 ptr(out), P + 2, ptr(mm), ptr(vv), 1, 1e-2, 0.9, 0.999, 1e-8, 0.0)
        small = lib.qhea_model_noisy_device_lds_grad_workspace_bytes(ctypes.byref(desc), 4, ctypes.byref(ok))
        assert small < need
        assert steps(*targs, ptr(ws), small, _lib._stream(dev)) == -3
        assert steps(*(targs[:9] + (None,) + targs[10:]), ptr(ws), need, _lib._stream(dev)) == -1
        assert untouched(st)
        assert call(ctypes.byref(desc), 0, 0, None, None, None, None, None, ctypes.byref(rec), ctypes.byref(ok), 0.1, None, None, None,
                    0, _lib._stream(dev)) == 0
        assert steps(*((targs[0], 0) + targs[2:]), None, 0, _lib._stream(dev)) == 0
    assert untouched(st)


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------

def test_device_trajectory_loss_and_grad(dev):
    from quanonet_amd import _lib
    from quanonet_amd.noise import Sampling, device_sampled_loss_and_grad, device_trajectory_loss_and_grad
    m = build('quanonet', 10, True, 'X', seed=2).to(dev)
    ins, y = _on(dev, inputs('quanonet', 4, seed=2), np.random.default_rng(2).normal(size=4))
    dn, sp = setting('strong', 10), Sampling(trajectories=3, seed=21)
    want, want_pred = _call(m, ins, y, dn, sp, row0=40)
    got, pred = device_trajectory_loss_and_grad(m, ins, y.reshape(-1, 1), dn, sp, row0=40)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(pred.cpu().numpy(), want_pred)
    want9, _ = _call(m, ins, y, dn, sp, inv=1.0 / 9)
    got9, _ = device_trajectory_loss_and_grad(m, ins, y, dn, sp, inv_batch_total=1.0 / 9)
    assert np.array_equal(got9.cpu().numpy(), want9)
    g0, p0 = device_trajectory_loss_and_grad(m, tuple(t[:0] for t in ins), y[:0], dn, sp)
    assert g0.abs().sum().item() == 0.0 and p0.numel() == 0
    with pytest.raises(ValueError, match='device_trajectory_loss_and_grad'):
        device_sampled_loss_and_grad(m, ins, y, dn, sp)
    # n = 8: the call of n = 7..9, bitwise
    m8 = build('heaqnn', 8, True, 'diag', seed=3).to(dev)
    ins8, y8 = _on(dev, inputs('heaqnn', 5, seed=4), np.random.default_rng(4).normal(size=5))
    dn8, sp8 = setting('strong', 8), Sampling(trajectories=5, seed=6)
    a, pa = device_sampled_loss_and_grad(m8, ins8, y8, dn8, sp8, row0=7)
    b, pb = device_trajectory_loss_and_grad(m8, ins8, y8, dn8, sp8, row0=7)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(pa, pb) and a[:-2].abs().max().item() > 1e-3


def test_ptsolver_trains_and_resumes(dev, tmp_path):
    """three epochs with train_device_noise + train_jump_trajectories at n = 10; the first step's loss is the single call's on the
    traced rows under stream seed + 1; the per-step path is the same run; and a trainer that takes over parameters, moments and
    the Adam count after epoch 1 reproduces epochs 2 and 3 bitwise"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import Sampling
    n = 10
    dn, sp = setting('strong', n, seed=4), Sampling(trajectories=TILE + 1, seed=2 ** 64 - 4)
    keys = dict(train_device_noise=dn.asdict(), train_jump_trajectories=sp.asdict(), num_qubits=n)
    s, hist, lines = _run(tmp_path, 'a', dev, **keys)
    assert s.trainer.device_sampled and s.trainer.train_device_noise == dn and s.trainer.train_sampling == sp
    assert s.trainer.sampling_key == 'train_jump_trajectories'
    assert sum('quantum-jump estimate' in ln for ln in lines) == 1
    nb = len(hist['loss_steps']) // 3
    assert len(hist['loss_train']) == 3 and nb >= 2 and all(np.isfinite(hist['loss_steps']))
    data = _solver_data()
    idx = np.asarray(hist['indices'][0])[:100]
    init = _run(tmp_path, 'init', dev, num_epochs=0, **keys)[0].model
    tens = lambda k, i: torch.tensor(np.asarray(data[k], np.float64)[i], device=dev)
    first = Sampling(trajectories=sp.trajectories, seed=(sp.seed + 1) % 2 ** 64)
    ref, _ = _call(init, (tens('train_branch_input', idx), tens('train_trunk_input', idx)), tens('train_output', idx)[:, 0], dn, first,
                   inv=1.0 / 100)
    assert abs(hist['loss_steps'][0] - ref[-2] / 100) < 1e-12
    _, ideal, _ = _run(tmp_path, 'ideal', dev, num_qubits=n)
    assert ideal['loss_steps'][0] != hist['loss_steps'][0]
    _, per_step, _ = _run(tmp_path, 'steps', dev, epoch_call=False, **keys)
    assert per_step['loss_steps'] == hist['loss_steps']
    # resumed after epoch 1
    s1, h1, _ = _run(tmp_path, 'one', dev, **dict(keys, num_epochs=1))
    assert h1['loss_steps'] == hist['loss_steps'][:nb]
    s2 = _run(tmp_path, 'rest', dev, **dict(keys, num_epochs=0))[0]
    t1, t2 = s1.trainer, s2.trainer
    t2.pflat.copy_(t1.pflat)
    t2.optimizer.exp_avg.copy_(t1.optimizer.exp_avg)
    t2.optimizer.exp_avg_sq.copy_(t1.optimizer.exp_avg_sq)
    t2.optimizer.t = t1.optimizer.t
    losses = []
    for ep in (1, 2):
        order = np.asarray(hist['indices'][ep])
        for a in range(0, len(order), 100):
            i = order[a:a + 100]
            flat = t2.train_step(tens('train_branch_input', i), tens('train_trunk_input', i), tens('train_output', i)[:, 0],
                                 global_batch=len(i), row0=a)
            losses.append(float(flat[-2]) / len(i))
    torch.cuda.synchronize()
    assert torch.equal(t2.pflat, s.trainer.pflat)
    assert losses == hist['loss_steps'][nb:]


def test_the_two_keys_are_one_run_at_n8(dev, tmp_path):
    from quanonet_amd.noise import Sampling
    dn, sp = setting('strong', 8, seed=1), Sampling(trajectories=5, seed=11)
    a, ha, _ = _run(tmp_path, 'old', dev, train_device_noise=dn.asdict(), train_trajectories=sp.asdict(), num_qubits=8, num_epochs=1)
    b, hb, _ = _run(tmp_path, 'new', dev, train_device_noise=dn.asdict(), train_jump_trajectories=sp.asdict(), num_qubits=8,
                    num_epochs=1)
    assert ha['loss_steps'] == hb['loss_steps'] and torch.equal(a.trainer.pflat, b.trainer.pflat)


def test_solver_refusals(dev, tmp_path):
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import DeviceNoise, Sampling
    from quanonet_amd.solver import DataParallelTrainer, PTSolver
    data = _solver_data()
    dn, sp = DeviceNoise(p1=0.01, t1=1.0, t2=1.0, t_rx=0.1, t_rot=0.1, t_cx=0.1).asdict(), Sampling(trajectories=4, seed=1)
    make = lambda name, **kw: PTSolver(_cfg(tmp_path, name, **kw), data, device=dev, log=quiet)
    with pytest.raises(ValueError, match='train_device_noise alone trains on the exact loss'):
        make('n6', train_device_noise=dn, train_jump_trajectories=sp, num_qubits=6)
    with pytest.raises(ValueError, match='train_jump_trajectories'):             # the old key at n >= 10 names the new one
        make('n10', train_device_noise=dn, train_trajectories=sp, num_qubits=10)
    with pytest.raises(ValueError, match='n = 7..9'):
        make('n10b', train_device_noise=dn, train_trajectories=sp, num_qubits=10)
    with pytest.raises(ValueError, match='both set'):
        make('two', train_device_noise=dn, train_trajectories=sp, train_jump_trajectories=sp, num_qubits=10)
    with pytest.raises(ValueError, match='both set'):
        make('two_s', train_device_noise=dn, train_sampling=sp, train_jump_trajectories=sp, num_qubits=10)
    with pytest.raises(ValueError, match='needs train_device_noise'):
        make('uniform', train_noise={'p1': 0.01}, train_jump_trajectories=sp, num_qubits=10)
    with pytest.raises(ValueError, match='needs train_device_noise'):
        make('bare', train_jump_trajectories=sp, num_qubits=10)
    with pytest.raises(ValueError, match='train_noise and train_device_noise'):
        make('both', train_device_noise=dn, train_noise={'p1': 0.01}, train_jump_trajectories=sp, num_qubits=10)
    with pytest.raises(ValueError, match='shots'):
        make('shots', train_device_noise=dn, train_jump_trajectories=Sampling(shots=10), num_qubits=10)
    with pytest.raises(ValueError, match='gamma = 1'):
        make('dead', train_device_noise=dict(dn, t1=1e-3, t2=1e-3), train_jump_trajectories=sp, num_qubits=10)
    with pytest.raises(ValueError, match='fused model-level path'):
        make('sgd', train_device_noise=dn, train_jump_trajectories=sp, optimizer='sgd', num_qubits=10)
    with pytest.raises(ValueError, match='world_size'):
        DataParallelTrainer(torch.nn.Linear(2, 1).double(), world_size=2, train_device_noise=dn, train_jump_trajectories=sp)
    for cls in (EnsembleSolver, DepthSweepSolver):
        cfgs = [_cfg(tmp_path, cls.__name__, seed=k, run_id=f'm{k}', num_qubits=2, train_jump_trajectories=sp) for k in (0, 1)]
        with pytest.raises(ValueError, match='train_jump_trajectories'):
            cls(cfgs, data, device=dev, log=quiet)
