"""
The quantum-jump trajectory gradient on the GPU (qhea_model_loss_grad_noisy_device / qhea_model_train_steps_noisy_device, through
quanonet_amd._lib and quanonet_amd.noise.device_sampled_loss_and_grad) against the numpy reference
tests/device_traj_grad_reference.py, which replays the header's random stream with the kernel's unnormalised rule: the whole
[P + 2] buffer and pred at n = 7, 8, 9 under four kinds of device setting, all rates zero = the ideal call, pred = the forward
call's, independence of the batch, train_steps = the loop of single calls, graph capture, unbiasedness against the CPU density
matrix (where the ideal and the relaxation-free derivatives fail), refusals, and the solver's keys.

Tolerance against the reference: atol 1e-10, the one qhea_model_loss_grad_noisy_wide is held to.  A jump decision
u N2 < gamma M differs between kernel and numpy only where u lies within a few ulps (1e-15 relative) of the edge: the cases
here make fewer than 1e5 decisions, a chance below 1e-10 over the set -- the argument of tests/test_device_traj.py.  No row is
excluded.
Shapes: two blocks per net, sub-layers per block 1 and 2; the kernel's tile is 4 trajectories, so T = 1, 4 and 5 are one short
tile, one full tile, and a full tile followed by a tile of one.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import device_noise_grad_reference as DG
from tests import device_traj_grad_reference as G
from tests import helpers as H
from tests import noisy_traj_grad_reference as TG
from tests.test_noisy_forward import _circuit, _solver_data
from tests.test_noisy_traj_grad_reference import build, inputs, within_sigmas

pytestmark = pytest.mark.gpu
ATOL = 1e-10
TILE = 4
BIG = (1 << 32) + 5                         # a global row index whose high counter word is in use
quiet = lambda *a, **k: None


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def setting(kind, n, idle=True, asym=True, seed=0):
    """the four kinds of device setting the walk must cover (the coverage is asserted from the replay in the tests)"""
    from quanonet_amd.noise import DeviceNoise
    rng = np.random.default_rng(3000 + 10 * n + seed)
    r01 = rng.uniform(0.01, 0.05, n)
    r10 = rng.uniform(0.04, 0.09, n) if asym else r01
    t1 = rng.uniform(0.8, 1.4, n)
    base = dict(p1=rng.uniform(0.02, 0.05, n), p2=rng.uniform(0.05, 0.1, n), readout01=r01, readout10=r10, idle=idle)
    if kind == 'none':                      # (i) no relaxation at all: gamma = 0, pz = 0
        return DeviceNoise(**base, t_rx=0.1, t_rot=0.1, t_cx=0.1)
    if kind == 'strong':                    # (ii) gamma of 0.3 and more at every site
        return DeviceNoise(**base, t1=t1, t2=t1 * rng.uniform(0.6, 1.8, n), t_rx=0.5, t_rot=0.4, t_cx=0.5)
    if kind == 'dephasing':                 # (iii) dephasing only
        return DeviceNoise(**base, t1=math.inf, t2=rng.uniform(0.5, 1.0, n), t_rx=0.2, t_rot=0.2, t_cx=0.3)
    assert kind == 'polar'                  # (iv) frequent X / Y errors in front of strong relaxation
    return DeviceNoise(**dict(base, p1=rng.uniform(0.3, 0.4, n), p2=rng.uniform(0.3, 0.4, n)), t1=t1, t2=t1, t_rx=0.5, t_rot=0.4,
                       t_cx=0.5)


def as_dict(dn, n):
    d = {k: [dn._at(k, q) for q in range(n)] for k in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2')}
    d.update(t_rx=dn.t_rx, t_rot=dn.t_rot, t_cx=dn.t_cx, idle=dn.idle)
    return d


def _diag(m):
    q = m.quantum_layer
    return q.ham_diag if q.use_full_ham else None


def _on(dev, ins, y):
    return tuple(torch.tensor(t, device=dev) for t in ins), torch.tensor(np.asarray(y, np.float64), device=dev)


def _call(m, ins, y, dn, sp, row0=0, inv=None, want_pred=True):
    """(grad[P+2], pred[B]) of one qhea_model_loss_grad_noisy_device call as numpy arrays; m, ins, y on the device"""
    from quanonet_amd import _lib
    flat = H.flat(m)
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device) if want_pred else None
    _lib.model_loss_grad_noisy_device(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat, dn.params(m.num_qubits),
                                      sp.params(), 1.0 / rows if inv is None else inv, grad, row0=row0, ham_diag=_diag(m),
                                      pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (pred.cpu().numpy() if want_pred else None)


def _coverage(cpu, ins, dn, T, seed, row0):
    c, _ = _circuit(cpu, tuple(torch.as_tensor(t) for t in ins))
    r = G.walk(c['n'], c['cfgs'], c['x'], c['w'], as_dict(dn, c['n']), T, seed, c['offset'], c['coeff'], c['ham_diag'],
               c['ham_pauli'], row0=row0, grad=False)
    return G.coverage(r, c['n'], T)


# every value of every axis at each n: model, frequency kind, read-out, setting, idle, readout asymmetric, row0, T
CASES = [('quanonet', True, 'Z', 'strong', True, True, 0, TILE + 1),
         ('heaqnn', False, 'X', 'none', False, False, BIG, TILE),
         ('quanonet', False, 'Y', 'dephasing', True, True, BIG, 1),
         ('heaqnn', True, 'diag', 'polar', False, True, 0, TILE + 1),
         ('heaqnn', True, 'diag', 'strong', False, False, BIG, TILE)]


@pytest.mark.parametrize('n', [7, 8, 9])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_against_the_reference(dev, n, case):
    from quanonet_amd.noise import Sampling
    kind, trainable, readout, what, idle, asym, row0, T = CASES[case]
    rows = 5                                                  # not a multiple of the four waves of a workgroup
    cpu = build(kind, n, trainable, readout, seed=n + case, net=(2, 1) if case == 4 else None)
    ins, y = inputs(kind, rows, seed=case), np.random.default_rng(n + case).normal(scale=0.7, size=rows)
    dn, sp = setting(what, n, idle, asym, seed=case), Sampling(trajectories=T, seed=1234 + case)
    # what the case is about happens in the compared rows, or it shows nothing
    cov = _coverage(cpu, ins, dn, T, sp.seed, row0)
    if what == 'none':
        assert cov['jumps'].size == rows * T and cov['jumps'].sum() == 0 and cov['dephasing'] == 0 and cov['pauli'] >= 1, cov
    elif what == 'dephasing':
        assert cov['jumps'].sum() == 0 and cov['dephasing'] >= rows * T, cov
    elif what == 'strong':
        assert cov['jumps'].min() >= 2 and cov['most_in_block'].max() >= 2, cov
        assert cov['first_enc'] >= 1 and cov['last_ctl'] >= 1 and cov['high_wire'] >= 1, cov
    else:
        assert cov['polarity'] >= 1 and cov['jumps'].min() >= 2, cov
    ref, ref_pred = TG.model_loss_grad(cpu, ins, y, 1.0 / 7, G.DeviceTrajEngine(as_dict(dn, n), T, sp.seed, row0))
    grad, pred = _call(cpu.to(dev), *_on(dev, ins, y), dn, sp, row0=row0, inv=1.0 / 7)
    tag = f'n={n} {kind} trainable={trainable} {readout} {what} idle={idle} asym={asym} row0={row0} T={T}'
    print(f'{tag}: max|grad err|={np.abs(grad - ref).max():.2e} max|pred err|={np.abs(pred - ref_pred).max():.2e} '
          f'max|grad|={np.abs(ref[:-2]).max():.2e} jumps={int(cov["jumps"].sum())} polarity={cov["polarity"]}')
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL, err_msg=tag)


@pytest.mark.parametrize('n', [7, 8, 9])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_all_rates_zero_equals_ideal(dev, n, kind):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise, Sampling
    for trainable, readout in ((True, 'Z'), (False, 'X'), (True, 'Y'), (False, 'diag')):
        m = build(kind, n, trainable, readout, seed=n).to(dev)
        rows = 37
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


@pytest.mark.parametrize('n,kind,readout', [(7, 'quanonet', 'Z'), (8, 'heaqnn', 'diag'), (9, 'quanonet', 'X'), (8, 'heaqnn', 'Y')])
def test_pred_is_the_forward_calls(dev, n, kind, readout):
    """same setting, sampling and row0: the two calls add the same trajectory values in different tiles (1e-13)"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import Sampling
    m = build(kind, n, True, readout, seed=n).to(dev)
    rows = 23
    ins, y = _on(dev, inputs(kind, rows, seed=2), np.zeros(rows))
    dn = setting('strong', n)
    for T, row0 in ((1, 0), (TILE + 1, BIG), (70, 5)):
        sp = Sampling(trajectories=T, seed=77)
        _, pred = _call(m, ins, y, dn, sp, row0=row0)
        fwd, _ = _lib.model_forward_noisy_device(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, H.flat(m), dn.params(n),
                                                 sp.params(), row0=row0, ham_diag=_diag(m))
        torch.cuda.synchronize()
        gap = np.abs(pred - fwd.cpu().numpy()).max()
        print(f'n={n} {kind} {readout} T={T}: max|pred - forward| = {gap:.2e}')
        assert gap <= 1e-13


@pytest.mark.parametrize('n,kind,readout', [(7, 'heaqnn', 'Z'), (8, 'quanonet', 'Y'), (9, 'heaqnn', 'diag')])
def test_a_row_does_not_depend_on_its_batch(dev, n, kind, readout):
    from quanonet_amd.noise import Sampling
    cpu, m = build(kind, n, True, readout, seed=4), build(kind, n, True, readout, seed=4).to(dev)
    rows, cut, base = 11, 4, BIG - 3
    ins, y0 = _on(dev, inputs(kind, rows, seed=8), np.zeros(rows))
    dn, sp = setting('strong', n, seed=2), Sampling(trajectories=TILE + 3, seed=5)
    g_all, pred = _call(m, ins, y0, dn, sp, row0=base)
    _, pa = _call(m, tuple(t[:cut] for t in ins), y0[:cut], dn, sp, row0=base)
    _, pb = _call(m, tuple(t[cut:] for t in ins), y0[cut:], dn, sp, row0=base + cut)
    assert np.array_equal(np.concatenate([pa, pb]), pred)
    g2, p2 = _call(m, ins, y0, dn, sp, row0=base)
    assert np.array_equal(g2, g_all) and np.array_equal(p2, pred)              # and a second call: bitwise
    # one row's record alone (y = pred elsewhere makes every other weight an exact zero): in the whole batch, in its part of
    # the split, and as a batch of one with its own row0
    for r in (1, 6, 10):
        y = torch.tensor(pred, device=dev)
        y[r] += 1.0
        whole, _ = _call(m, ins, y, dn, sp, row0=base, inv=0.5)
        lo, hi = (0, cut) if r < cut else (cut, rows)
        part, _ = _call(m, tuple(t[lo:hi] for t in ins), y[lo:hi], dn, sp, row0=base + lo, inv=0.5)
        alone, _ = _call(m, tuple(t[r:r + 1] for t in ins), y[r:r + 1], dn, sp, row0=base + r, inv=0.5)
        assert np.array_equal(whole[:-2], part[:-2]) and np.array_equal(whole[:-2], alone[:-2]), r
        assert np.abs(whole[:-2]).max() > 1e-3
    other, _ = _call(m, tuple(t[r:r + 1] for t in ins), y[r:r + 1] + 1.0, dn, sp, row0=base + r, inv=0.5)
    ref = TG.dpred(cpu, tuple(t[r:r + 1].cpu().numpy() for t in ins), G.DeviceTrajEngine(as_dict(dn, n), sp.trajectories, sp.seed,
                                                                                         base + r))
    np.testing.assert_allclose((alone - other)[:-2], ref, rtol=0, atol=ATOL)


def test_more_items_than_waves(dev):
    """2200 (row, tile) items on 2048 waves: the grid-stride loop takes a second round, and a row's result is the one it has
    in a small batch"""
    from quanonet_amd.noise import Sampling
    m = build('heaqnn', 7, True, 'Z', seed=1, net=(1, 1)).to(dev)
    rows = 1100
    ins, y0 = _on(dev, inputs('heaqnn', rows, seed=3), np.zeros(rows))
    dn, sp = setting('strong', 7), Sampling(trajectories=2 * TILE, seed=9)
    _, pred = _call(m, ins, y0, dn, sp, row0=0)
    for lo in (0, 1020, 1096):
        _, part = _call(m, tuple(t[lo:lo + 4] for t in ins), y0[lo:lo + 4], dn, sp, row0=lo)
        assert np.array_equal(part, pred[lo:lo + 4])
    y = torch.tensor(pred, device=dev)
    y[1099] += 1.0
    whole, _ = _call(m, ins, y, dn, sp, inv=0.5)
    alone, _ = _call(m, tuple(t[1099:] for t in ins), y[1099:], dn, sp, row0=1099, inv=0.5)
    assert np.array_equal(whole[:-2], alone[:-2]) and np.abs(whole[:-2]).max() > 1e-3


UNBIASED = dict(n=7, net=(1, 1), T=64, seeds=tuple(range(100, 116)), sigmas=5.0)


def test_unbiasedness(dev):
    """n = 7, HEAQNN, one block, one row, 16 seeds of 64 trajectories under strong relaxation: every component of the seeds' mean
    of d pred / d params within 5 standard errors (across the seeds) of the exact derivative -- central differences at +- pi / 2
    of tests/device_noise_reference.py's 128 x 128 density matrix.  The ideal derivative and the derivative under the same
    Pauli and readout rates without relaxation both fail the same check."""
    from quanonet_amd.noise import DeviceNoise, Sampling
    u = UNBIASED
    cpu, ins_np = build('heaqnn', u['n'], True, 'Z', seed=3, net=u['net']), inputs('heaqnn', 1, seed=11)
    # gamma = 0.13 .. 0.31 per site: jumps are common and the state is not driven to |0..0>, so the derivative still scatters
    t1 = np.random.default_rng(1).uniform(0.8, 1.4, u['n'])
    dn = DeviceNoise(p1=0.01, p2=0.02, readout01=0.02, readout10=0.05, t1=t1, t2=0.9 * t1, t_rx=0.2, t_rot=0.2, t_cx=0.3, idle=False)
    nz = as_dict(dn, u['n'])
    shift = lambda d: TG._Engine(lambda n, cfgs, x, w, off, co, hd, hp: DG.shift_grad(n, cfgs, x, w, d, off, co, hd, hp))
    exact = TG.dpred(cpu, ins_np, shift(nz))
    ideal = TG.dpred(cpu, ins_np, None)
    no_relax = TG.dpred(cpu, ins_np, shift(dict(nz, t1=[math.inf] * u['n'], t2=[math.inf] * u['n'])))
    m = cpu.to(dev)
    ins, y0 = _on(dev, ins_np, np.zeros(1))
    per_seed = []
    for s in u['seeds']:
        sp = Sampling(trajectories=u['T'], seed=s)
        g0, _ = _call(m, ins, y0, dn, sp, inv=0.5, want_pred=False)
        g1, _ = _call(m, ins, y0 + 1.0, dn, sp, inv=0.5, want_pred=False)
        per_seed.append((g0 - g1)[:-2])
    ok, worst = within_sigmas(per_seed, exact, u['sigmas'])
    _, worst_ideal = within_sigmas(per_seed, ideal, u['sigmas'])
    _, worst_no_relax = within_sigmas(per_seed, no_relax, u['sigmas'])
    print(f"16 x {u['T']}: worst deviation {worst:.2f} standard errors over {exact.size} components; ideal {worst_ideal:.1f}, "
          f"no relaxation {worst_no_relax:.1f}")
    assert exact.size == sum(p.numel() for p in m.parameters())                # no component left out
    assert ok, worst
    assert worst_ideal > u['sigmas'] and worst_no_relax > u['sigmas']


def _adam_state(flat):
    return flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)


@pytest.mark.parametrize('n,kind,readout,trainable', [(7, 'quanonet', 'Z', True), (8, 'heaqnn', 'diag', True),
                                                      (9, 'quanonet', 'X', False)])
def test_train_steps(dev, n, kind, readout, trainable):
    from quanonet_amd import _lib
    from quanonet_amd.noise import Sampling
    m = build(kind, n, trainable, readout, seed=5).to(dev)
    bounds, sizes = [0, 5, 12, 15], [5, 7, 3]
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
        _lib.model_train_steps_noisy_device(desc, bounds, sizes, ins[0], trunk, y, p1, out1, m1, v1, first, lr, b1, b2, eps, wd,
                                            dn.params(n), base.params(), ham_diag=diag)
        p2, m2, v2 = _adam_state(H.flat(m))
        out2 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
        for i in range(3):
            a, b = bounds[i], bounds[i + 1]
            sp = Sampling(trajectories=TILE + 1, seed=(base.seed + first + i) % 2 ** 64)
            _lib.model_loss_grad_noisy_device(desc, ins[0][a:b], None if trunk is None else trunk[a:b], y[a:b], p2, dn.params(n),
                                              sp.params(), 1.0 / sizes[i], out2[i], row0=a, ham_diag=diag)
            _lib.adam_step(p2, out2[i], m2, v2, first + i, lr, b1, b2, eps, wd)
        torch.cuda.synchronize()
        assert torch.equal(out1, out2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2), first
        assert not torch.equal(p1, H.flat(m))
        firsts[first] = out1[0].cpu().numpy()
    assert not np.array_equal(firsts[1][:P], firsts[5][:P])                      # fresh draws per Adam count
    assert firsts[1][P + 1] == firsts[5][P + 1]


def test_refusals_leave_the_outputs_untouched(dev):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    from tests.test_device_noise_abi import _record
    m = build('quanonet', 7, True, 'Z').to(dev)
    ins, y = _on(dev, inputs('quanonet', 10), np.random.default_rng(0).normal(size=10))
    desc, params = m.fused_desc(), H.flat(m)
    P = params.numel()
    dn, ok = setting('strong', 7), _lib.SamplingParams(0, 20, 1)
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
                _lib.model_loss_grad_noisy_device(d, i[0], tr, y, p, rec, sp, 0.1, g, pred=pr)
        with pytest.raises(exc, match=match):
            _lib.model_train_steps_noisy_device(d, [0, 4, 10], [4, 6], i[0], tr, y, p, out, mm, vv, first_step, 1e-2, 0.9, 0.999,
                                                1e-8, 0.0, rec, sp)
        assert untouched(st)

    for bad in (_lib.SamplingParams(1, 20, 1), _lib.SamplingParams(0, 0, 1), _lib.SamplingParams(-1, 20, 1)):
        both(desc, ins, _lib.QheaError, dn.params(7), bad)                        # shots = 1, trajectories = 0
    both(desc, ins, _lib.QheaError, _record(7, p1=[1.5] * 7), ok)                 # a bad device setting
    both(desc, ins, _lib.QheaError, dn.params(7), ok, trunk=None)                 # a QuanONet without its trunk input
    both(desc, ins, _lib.QheaError, dn.params(7), ok, first_step=0)
    # a site with gamma = 1: named in the message
    dead = DeviceNoise(t1=[1.0] * 6 + [1e-3], t2=[1.0] * 6 + [1e-3], t_rx=0.001, t_rot=0.001, t_cx=0.1, idle=False)
    both(desc, ins, _lib.QheaError, dead.params(7), ok, match='CTL on wire 6')
    for n in (6, 10):
        mn = build('heaqnn', n, True, 'Z').to(dev)
        xn, pn = torch.tensor(inputs('heaqnn', 10)[0], device=dev), H.flat(mn)
        gn, prn = torch.full((pn.numel() + 2,), 123.0, dtype=torch.float64, device=dev), torch.full((10,), 456.0, dtype=torch.float64, device=dev)
        mmn, vvn, outn = torch.full_like(pn, 7.0), torch.full_like(pn, 8.0), torch.full((2, pn.numel() + 2), 123.0, dtype=torch.float64, device=dev)
        with pytest.raises(_lib.Unsupported):
            _lib.model_loss_grad_noisy_device(mn.fused_desc(), xn, None, y, pn, setting('strong', n).params(n), ok, 0.1, gn, pred=prn)
        with pytest.raises(_lib.Unsupported):
            _lib.model_train_steps_noisy_device(mn.fused_desc(), [0, 4, 10], [4, 6], xn, None, y, pn, outn, mmn, vvn, 1, 1e-2, 0.9,
                                                0.999, 1e-8, 0.0, setting('strong', n).params(n), ok)
        torch.cuda.synchronize()
        assert torch.all(gn == 123.0) and torch.all(prn == 456.0) and torch.all(outn == 123.0) and torch.equal(pn, H.flat(mn))
        assert torch.all(mmn == 7.0) and torch.all(vvn == 8.0)
    # a NULL sampling and a workspace one byte short, through the C ABI itself
    lib = _lib.load()
    rec = dn.params(7)
    need = lib.qhea_model_noisy_device_grad_workspace_bytes(ctypes.byref(desc), 10, ctypes.byref(ok))
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    st = state()
    g, pr, p, mm, vv, out = st
    ptr = _lib._ptr
    with torch.cuda.device(dev):
        head = (ctypes.byref(desc), 0, 10, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(p), None, ctypes.byref(rec))
        tail = (0.1, ptr(g), ptr(pr))
        assert lib.qhea_model_loss_grad_noisy_device(*head, None, *tail, ptr(ws), need, _lib._stream(dev)) == -1
        assert lib.qhea_model_loss_grad_noisy_device(*head, ctypes.byref(ok), *tail, ptr(ws), need - 1, _lib._stream(dev)) == -3
        assert lib.qhea_model_loss_grad_noisy_device(*head, ctypes.byref(ok), *tail, None, 0, _lib._stream(dev)) == -3
        rb, ib = (ctypes.c_int64 * 3)(0, 4, 10), (ctypes.c_double * 2)(0.25, 1.0 / 6)
        targs = (ctypes.byref(desc), 2, rb, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(p), None, ctypes.byref(rec), ctypes.byref(ok), ib,
                 ptr(out), P + 2, ptr(mm), ptr(vv), 1, 1e-2, 0.9, 0.999, 1e-8, 0.0)
        small = lib.qhea_model_noisy_device_grad_workspace_bytes(ctypes.byref(desc), 4, ctypes.byref(ok))
        assert lib.qhea_model_train_steps_noisy_device(*targs, ptr(ws), small, _lib._stream(dev)) == -3
        assert lib.qhea_model_train_steps_noisy_device(*(targs[:9] + (None,) + targs[10:]), ptr(ws), need, _lib._stream(dev)) == -1
        assert untouched(st)
        assert lib.qhea_model_loss_grad_noisy_device(ctypes.byref(desc), 0, 0, None, None, None, None, None, ctypes.byref(rec),
                                                     ctypes.byref(ok), 0.1, None, None, None, 0, _lib._stream(dev)) == 0
        assert lib.qhea_model_train_steps_noisy_device(*((targs[0], 0) + targs[2:]), None, 0, _lib._stream(dev)) == 0
    assert untouched(st)


@pytest.mark.parametrize('readout', ['Z', 'diag'])
def test_graph_capture_and_launch_count(dev, readout):
    """per call the kernel that writes the per-site constants and h', per step the prep kernel, the trajectory kernel, the fold
    kernel and the reduce kernel (include/quanonet_hea.h)"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import Sampling
    m = build('heaqnn', 8, True, readout, seed=1).to(dev)
    bounds, sizes = [0, 9], [9]
    ins, y = _on(dev, inputs('heaqnn', 9), np.random.default_rng(2).normal(size=9))
    desc, diag = m.fused_desc(), _diag(m)
    dn, sp = setting('strong', 8).params(8), Sampling(trajectories=TILE + 1, seed=8).params()
    P = H.flat(m).numel()

    def run(st):
        p, mm, vv, out = st
        _lib.model_train_steps_noisy_device(desc, bounds, sizes, ins[0], None, y, p, out, mm, vv, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0, dn,
                                            sp, ham_diag=diag)

    fresh = lambda: (*_adam_state(H.flat(m)), torch.zeros(1, P + 2, dtype=torch.float64, device=dev))
    eager = fresh()
    run(eager)                                                                     # also sizes the workspace outside the capture
    torch.cuda.synchronize()
    scratch = fresh()
    names = [k[0] for k in H.kernel_launches(dev, lambda: run(scratch))]
    want = ['device_grad_tables_kernel', 'prep_model_kernel', 'device_grad_wave_kernel', 'noisy_grad_fold_kernel',
            'reduce_density_kernel']
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
    assert not torch.equal(eager[0], H.flat(m))


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------

def test_device_sampled_loss_and_grad(dev):
    from quanonet_amd.noise import Sampling, device_sampled_loss_and_grad
    m = build('quanonet', 7, True, 'X', seed=2).to(dev)
    ins, y = _on(dev, inputs('quanonet', 6, seed=2), np.random.default_rng(2).normal(size=6))
    dn, sp = setting('strong', 7), Sampling(trajectories=6, seed=21)
    want, want_pred = _call(m, ins, y, dn, sp, row0=40)
    got, pred = device_sampled_loss_and_grad(m, ins, y.reshape(-1, 1), dn, sp, row0=40)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(pred.cpu().numpy(), want_pred)
    want9, _ = _call(m, ins, y, dn, sp, inv=1.0 / 9)
    got9, _ = device_sampled_loss_and_grad(m, ins, y, dn, sp, inv_batch_total=1.0 / 9)
    assert np.array_equal(got9.cpu().numpy(), want9)
    g0, p0 = device_sampled_loss_and_grad(m, tuple(t[:0] for t in ins), y[:0], dn, sp)
    assert g0.abs().sum().item() == 0.0 and p0.numel() == 0


def _cfg(tmp_path, name, **kw):
    cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': 7, 'net_size': [2, 1, 1, 1], 'scale_coeff': 0.5,
           'if_trainable_freq': 'true', 'learning_rate': 2e-2, 'batch_size': 100, 'num_epochs': 3, 'seed': 0,
           'prefix': str(tmp_path / name), 'run_id': 'r0', 'eval_batch_size': 64, 'trace_steps': True, 'if_save': False}
    cfg.update(kw)
    return cfg


def _run(tmp_path, name, dev, **kw):
    from quanonet_amd.solver import PTSolver, set_random_seed
    set_random_seed(0)
    lines = []
    s = PTSolver(_cfg(tmp_path, name, **kw), _solver_data(), device=dev, log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return s, s.train(), lines


def test_ptsolver_trains_and_resumes(dev, tmp_path):
    """three epochs with train_device_noise + train_trajectories at n = 7; the per-step path is the same run; and a trainer that
    takes over parameters, moments and the Adam count after epoch 1 reproduces epochs 2 and 3 bitwise (the stream is keyed by
    seed + Adam count, the rows by their place in the epoch)"""
    from quanonet_amd.noise import Sampling
    dn, sp = setting('strong', 7, seed=4), Sampling(trajectories=TILE + 1, seed=2 ** 64 - 4)
    keys = dict(train_device_noise=dn.asdict(), train_trajectories=sp.asdict())
    s, hist, lines = _run(tmp_path, 'a', dev, **keys)
    assert s.trainer.device_sampled and s.trainer.train_device_noise == dn and s.trainer.train_sampling == sp
    assert sum('quantum-jump estimate' in ln for ln in lines) == 1
    nb = len(hist['loss_steps']) // 3
    assert len(hist['loss_train']) == 3 and nb >= 2 and all(np.isfinite(hist['loss_steps']))
    # the first step's loss is the header's: the reference on the traced rows, stream seed + 1
    idx = np.asarray(hist['indices'][0])[:100]
    init = _run(tmp_path, 'init', dev, num_epochs=0, **keys)[0].model
    data = _solver_data()
    ref, _ = TG.model_loss_grad(init.cpu(), (data['train_branch_input'][idx], data['train_trunk_input'][idx]),
                                data['train_output'][idx, 0], 1.0 / 100,
                                G.DeviceTrajEngine(as_dict(dn, 7), sp.trajectories, (sp.seed + 1) % 2 ** 64, 0))
    assert abs(hist['loss_steps'][0] - ref[-2] / 100) < 1e-9
    _, ideal, _ = _run(tmp_path, 'ideal', dev)
    assert ideal['loss_steps'][0] != hist['loss_steps'][0]
    _, per_step, _ = _run(tmp_path, 'steps', dev, epoch_call=False, **keys)
    assert per_step['loss_steps'] == hist['loss_steps']
    # resumed after epoch 1
    s1, h1, _ = _run(tmp_path, 'one', dev, num_epochs=1, **keys)
    assert h1['loss_steps'] == hist['loss_steps'][:nb]
    s2 = _run(tmp_path, 'rest', dev, num_epochs=0, **keys)[0]
    t1, t2 = s1.trainer, s2.trainer
    t2.pflat.copy_(t1.pflat)
    t2.optimizer.exp_avg.copy_(t1.optimizer.exp_avg)
    t2.optimizer.exp_avg_sq.copy_(t1.optimizer.exp_avg_sq)
    t2.optimizer.t = t1.optimizer.t
    tens = lambda k, i: torch.tensor(np.asarray(data[k], np.float64)[i], device=dev)
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


def test_solver_refusals(dev, tmp_path):
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import DeviceNoise, Sampling
    from quanonet_amd.solver import DataParallelTrainer, PTSolver
    data = _solver_data()
    dn, sp = DeviceNoise(p1=0.01, t1=1.0, t2=1.0, t_rx=0.1, t_rot=0.1, t_cx=0.1).asdict(), Sampling(trajectories=4, seed=1)
    make = lambda name, **kw: PTSolver(_cfg(tmp_path, name, **kw), data, device=dev, log=quiet)
    with pytest.raises(ValueError, match='train_device_noise alone trains on the exact loss'):
        make('n6', train_device_noise=dn, train_trajectories=sp, num_qubits=6)
    with pytest.raises(ValueError, match='n = 7..9'):
        make('n10', train_device_noise=dn, train_trajectories=sp, num_qubits=10)
    with pytest.raises(ValueError, match='train_trajectories is the key'):
        make('sampling', train_device_noise=dn, train_sampling=sp)
    with pytest.raises(ValueError, match='train_noise and train_device_noise'):
        make('both', train_device_noise=dn, train_noise={'p1': 0.01}, train_trajectories=sp)
    with pytest.raises(ValueError, match='shots'):
        make('shots', train_device_noise=dn, train_trajectories=Sampling(shots=10))
    with pytest.raises(ValueError, match='train_trajectories beside train_device_noise'):
        make('alone', train_device_noise=dn)
    with pytest.raises(ValueError, match='gamma = 1'):
        make('dead', train_device_noise=dict(dn, t1=1e-3, t2=1e-3), train_trajectories=sp)
    with pytest.raises(ValueError, match='fused model-level path'):
        make('sgd', train_device_noise=dn, train_trajectories=sp, optimizer='sgd')
    with pytest.raises(ValueError, match='world_size'):
        DataParallelTrainer(torch.nn.Linear(2, 1).double(), world_size=2, train_device_noise=dn, train_trajectories=sp)
    for cls in (EnsembleSolver, DepthSweepSolver):
        cfgs = [_cfg(tmp_path, cls.__name__, seed=k, run_id=f'm{k}', num_qubits=2, train_device_noise=dn, train_trajectories=sp)
                for k in (0, 1)]
        with pytest.raises(ValueError, match='train_device_noise'):
            cls(cfgs, data, device=dev, log=quiet)
