"""
The extended-precision walks and the case table of the trajectory gradient budgets (tests/traj_precision_cases.py).  CPU only.

* threading a dtype through the trajectory references changed no fp64 result: one small call per routine, bit for bit against
  values the routines gave before they took a dtype (tests/golden/traj_reference_fp64_pins.npz);
* per case, from the references alone: the wide walk is wide and reproduces the fp64 walk, the residuals do not cancel,
  budget(row) <= 2^-10 max|row_ld|, and in the jump family every jump and rescale decision of the wide walk is 2^-40 (relative)
  clear of its threshold and the wide and the fp64 walk fire the same pattern;
* every jump case's LEVEL lies in its window; the realistic level and the level about 2 get no restart from the tabled rule
  (restart_above=RESTART_TABLED), the levels past 12 do; the polar case fires under an X of the frame, the rescale case crosses
  2^-200;
* the sampled family has the README's rates at the four shapes, the heavy rates at n = 7 and n = 10, a trainable-frequency
  QuanONet at n = 9 and all four read-outs;
* the wide adjoint walk agrees with the wide two-term shift on the first block of the n = 7 cases (both sampled ones and the
  realistic jump one), to a tolerance made
  of the wide type's epsilon and the operation count (at larger D or smaller N2 that tolerance is coarser than fp64);
* the finding: on the past-12 case at n = 7 the fp64 inverse walk WITHOUT a restart -- the kernels' rule -- is off by more than
  the budget, the stored walk and the restarted inverse walk are inside it; quanonet_amd.noise refuses that setting.

Run time, one core: 45 s for this file against 46 s for tests/test_density_precision_oracle.py in the same run (11 s of it the
six sampled cases; a full shift instead of traj_precision_cases.SHIFTED_ANGLES angles would add 160 s).
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from oracle.ld_oracle import err
from tests import device_traj_grad_reference as G
from tests import device_traj_reference as DT
from tests import helpers as H
from tests import noise_oracle as NO
from tests import noisy_traj_grad_reference as NTG
from tests import traj_precision_cases as TP

IDS = [c.id for c in TP.CASES]
JUMP = [c for c in TP.CASES if c.family == 'jump']
EPS = float(np.finfo(np.longdouble).eps)             # 2^-63 on x86


def test_table():
    assert len(set(IDS)) == len(IDS)
    by = lambda fam: [c for c in TP.CASES if c.family == fam]
    shapes = {(n, net) for n, net in TP.SHAPES}
    blocks = lambda c: (c.n, (c.net[0] + c.net[2], c.net[1]) if c.kind == 'quanonet' else c.net)
    assert {blocks(c) for c in by('sampled')} == shapes and {blocks(c) for c in JUMP if c.level} == shapes
    assert {c.readout for c in JUMP} == {'Z', 'X', 'Y', 'diag'} and {c.readout for c in by('sampled')} == {'Z', 'X', 'Y', 'diag'}
    # the README's rates at every shape, the heavy setting at n = 7 and at n = 10, one trainable-frequency QuanONet
    assert {c.n for c in by('sampled') if c.rates == TP.README_RATES} == {7, 9, 10, 12}
    assert {c.n for c in by('sampled') if c.rates == TP.HEAVY_RATES} == {7, 10} and TP.HEAVY_RATES == (0.05, 0.1)
    assert [c.n for c in by('sampled') if c.kind == 'quanonet'] == [9]
    assert all(c.rows == (1 if c.n == 12 or c.family == 'jump' else 2) for c in TP.CASES) and TP.T == 5
    # every level at every shape, but for what LOWERED lists
    have = {(blocks(c), c.level) for c in JUMP if c.level}
    for n, net in TP.SHAPES:
        for level in TP.LEVELS:
            assert ((n, net), level) in have or f'jump-q{n}-{net[0]}x{net[1]}-{level}' in TP.LOWERED, (n, level)
    assert sum(c.polar for c in JUMP) == 1 and sum(c.id.endswith('rescale') for c in JUMP) == 1
    name = '_ZN4qhea12_GLOBAL__N_123device_grad_wave_kernelILi7EEEvNS_13NoisyGradArgsENS0_11DevGradArgsE'
    assert TP._is(H.mangled_is, name, 'device_grad_wave_kernel', (7,)) and not TP._is(H.mangled_is, name, 'device_grad_wave_kernel', (8,))
    assert not TP._is(H.mangled_is, name, 'noisy_grad_wave_kernel') and not TP._is(H.mangled_is, name, 'device_grad_lds_kernel')


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 references are bit for bit what they were
# ---------------------------------------------------------------------------------------------------------------------
def pinned_calls():
    """{name: fp64 array} of one small call per routine that took a dtype, on fixed inputs (durations 0.05, 0.07, 0.21 and
    T1 / T2 of 1, 1.5, 4, inf: numpy's exp gives the same bits for them with and without its AVX-512 kernels)"""
    n, cfgs = 3, [(3, 1), (3, 2)]
    rng = np.random.default_rng(3600)
    x = rng.uniform(-2.0, 2.0, (2, 6))
    w = rng.uniform(-np.pi, np.pi, (3, 3, n))
    diag = rng.normal(size=1 << n)
    noise = SimpleNamespace(p1=0.05, p2=0.1, readout=0.03, shots=0, trajectories=3, seed=7)
    nz = dict(p1=[0.02, 0.03, 0.01], p2=[0.05, 0.04, 0.06], readout01=[0.01, 0.02, 0.01], readout10=[0.03, 0.04, 0.02],
              t1=[1.0, float('inf'), 1.5], t2=[1.5, 4.0, 1.0], t_rx=0.05, t_rot=0.06999999999999999, t_cx=0.21000000000000002,
              idle=True)
    out = {}
    out['sampled_replay'] = NO.replay_values(n, cfgs, x, w, noise, 0.3, 1.2, None, 'Y', 2)
    for k, v in zip('vxw', NTG.traj_grad(n, cfgs, x, w, noise, 0.3, 1.2, None, 'Y', 2)):
        out['sampled_walk_' + k] = v
    for k, v in zip('vxw', NTG.traj_grad_shift(n, cfgs, x, w, noise, 0.0, 1.0, diag, 'Z', 1)):
        out['sampled_shift_' + k] = v
    out['jump_replay'] = DT.replay_values(n, cfgs, x, w, nz, 0, 3, 5, 0.3, 1.2, None, 'X', 2)
    out['jump_pairs'] = DT.jump_pairs(n, nz)
    r = G.walk(n, cfgs, x, w, nz, 3, 5, 0.3, 1.2, None, 'X', 2)
    for k in ('value', 'num', 'N2', 'gx', 'gw'):
        out['jump_walk_' + k] = r[k]
    out['jump_walk_pattern'] = np.stack(r['pattern'])
    r = G.walk(n, cfgs, x, w, nz, 3, 5, 0.0, 1.0, diag, 'Z', 0, naive=True)
    for k in ('value', 'gx', 'gw'):
        out['jump_naive_' + k] = r[k]
    gx, gw = G.shift_grad(n, [(3, 1)], x[:, :3], w[:1], nz, 2, 5, 0.3, 1.2, None, 'Y', 1)
    out['jump_shift_gx'], out['jump_shift_gw'] = gx, gw
    # the model around the circuit, through the engines
    m = H.heaqnn(n, 2, (2, 1), 4, ham_pauli='Y')
    xin, y = rng.uniform(-1, 1, (3, 2)), rng.normal(size=3)
    for name, eng in (('sampled', NTG.TrajEngine(noise, row0=1)), ('jump', G.DeviceTrajEngine(nz, 3, 5, row0=1))):
        buf, pred = NTG.model_loss_grad(m, (xin,), y, 1.0 / 7, eng)
        out[name + '_model_buf'], out[name + '_model_pred'] = buf, pred
    q = H.quanonet(n, 3, 2, (1, 2, 1, 1), 2, scale_coeff=0.7, if_trainable_freq=False)
    br, tr = rng.uniform(-1, 1, (2, 3)), rng.uniform(-1, 1, (2, 2))
    buf, pred = NTG.model_loss_grad(q, (br, tr), y[:2], 0.5, G.DeviceTrajEngine(nz, 2, 9))
    out['jump_quanonet_buf'], out['jump_quanonet_pred'] = buf, pred
    return {k: np.asarray(v) for k, v in out.items()}, (m, xin, y, noise, nz)


def test_fp64_references_are_bitwise_unchanged():
    g = np.load(os.path.join(H.GOLDEN, 'traj_reference_fp64_pins.npz'))
    now, (m, xin, y, noise, nz) = pinned_calls()
    assert sorted(now) == sorted(g.files)
    for k, v in now.items():
        assert v.dtype == g[k].dtype and np.array_equal(v, g[k]), k
    # and the wide walks are the same functions: they differ from the pins by fp64 rounding only, in a wide array
    for name, eng in (('sampled', NTG.TrajEngine(noise, row0=1, dtype=TP.WIDE)),
                      ('sampled', NTG.TrajEngine(noise, row0=1, form=NTG.traj_grad_shift, dtype=TP.WIDE)),
                      ('jump', G.DeviceTrajEngine(nz, 3, 5, row0=1, dtype=TP.WIDE)),
                      ('jump', G.DeviceTrajEngine(nz, 3, 5, row0=1, dtype=TP.WIDE, inverse=True, restart_above=0.01))):
        buf, pred = NTG.model_loss_grad(m, (xin,), y, 1.0 / 7, eng, dtype=TP.WIDE)
        assert buf.dtype == np.longdouble and pred.dtype == np.longdouble
        assert 0 < np.abs(buf - g[name + '_model_buf']).max() < 1e-13 and np.abs(pred - g[name + '_model_pred']).max() < 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# the references and the conditions on the inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TP.CASES, ids=IDS)
def test_references_and_the_conditions_on_the_inputs(case):
    ref = TP.reference(case)
    names = ('adjoint walk', 'shift') if case.family == 'sampled' else ('stored walk', 'inverse walk')
    for q in TP.QUANTITIES:
        hi, lo = ref.ld[q]
        peak = TP._maxabs(hi)
        print(f'{case.id} {q}: e_ref {TP.e_ref(ref, q):.2e} ({names[0]} {ref.e_c[q]:.2e}, {names[1]} {ref.e_np[q]:.2e})  '
              f'budget {TP.budget(ref, q):.2e}  max|q| {peak:.2e}  budget / max|q| {TP.budget(ref, q) / peak:.2e}')
        assert np.isfinite(hi).all() and np.isfinite(lo).all()
        assert (np.abs(lo) <= np.spacing(np.abs(hi))).all(), q                # lo is what hi leaves over: the walk was wide
    assert TP._maxabs(ref.ld['row'][1]) > 0.0                                 # ... and carries more than 53 bits
    # the wide walk is the fp64 walk: they differ by what fp64 loses, far below any figure a test of the kernels has used
    assert ref.e_c['row'] <= 1e-10 * max(1.0, TP._maxabs(ref.ld['row'][0])), ref.e_c
    # the residuals do not cancel: the row is not made of pred's last bits (tests/density_precision_cases.py, SEEDS)
    pred, y = ref.ld['pred'][0], np.asarray(ref.inputs.y)
    assert (np.abs(pred - y) >= np.abs(pred) / 8).all(), (pred, y)
    # not vacuous: the budget resolves at least three digits of the largest gradient entry
    assert TP.budget(ref, 'row') <= 2.0 ** -10 * TP._maxabs(ref.ld['row'][0])
    if case.family == 'jump':
        wide, f64 = TP.pattern_walk(case, dtype=TP.WIDE), TP.pattern_walk(case)
        print(f'{case.id}: margins {wide["margin"]}  jumps {f64["counts"]["jump"]}  rescales {f64["rescaled"]}')
        assert wide['margin']['jump'] >= 2.0 ** -40 and wide['margin']['rescale'] >= 2.0 ** -40, wide['margin']
        assert len(wide['pattern']) == len(f64['pattern'])
        assert all(np.array_equal(a, b) for a, b in zip(wide['pattern'], f64['pattern']))


@pytest.mark.parametrize('case', JUMP, ids=lambda c: c.id)
def test_levels_and_coverage(case):
    i = TP.inputs_of(case)
    x, w, ro = TP.circuit_of(case)
    r = G.walk(case.n, TP.cfgs_of(case), x, w, i.nz, TP.T, case.seed, row0=case.row0, inverse=True,
               restart_above=G.RESTART_TABLED, **ro)
    cov = G.coverage(r, case.n, TP.T)
    level, gammas = float(r['level'].max()), DT.jump_pairs(case.n, i.nz)[..., 0]
    print(f'{case.id}: LEVEL {level:.2f} (per trajectory {np.round(r["level"], 2)})  gamma {gammas.min():.2e} .. {gammas.max():.6f}  '
          f'jumps {cov["jumps"]}  restarts {r["restarts"]}  rescales {r["rescaled"]}  under X {cov["polarity"]}')
    if case.level:
        lo, hi = TP.LEVELS[case.level]
        assert lo <= level < hi, (level, case.level)
    if case.level == 'low':
        assert 1e-3 <= gammas.min() and gammas.max() <= 0.06 and i.nz['idle']     # a realistic calibration
    if case.level in ('low', 'L2'):
        assert r['restarts'].sum() == 0
    if case.level == 'past12':
        assert r['restarts'].sum() >= 1
    if case.polar:
        assert cov['polarity'] >= 1
    if case.id.endswith('rescale'):
        assert r['rescaled'].min() >= 1
    assert cov['jumps'].sum() >= 1 or case.level == 'low'


# ---------------------------------------------------------------------------------------------------------------------
# the wide adjoint walks against the wide two-term shift
# ---------------------------------------------------------------------------------------------------------------------
def _first_block(case):
    x, w, ro = TP.circuit_of(case)
    n, ld = case.n, case.net[1]
    return [(n, ld)], x[:1, :n], w[:ld], ro


SHIFTED = [c for c in TP.CASES if c.n == 7 and (c.level == 'low' or c.kind == 'heaqnn' and c.family == 'sampled')]    # where the tolerance below is finer than fp64: min N2 near 1, D = 128


@pytest.mark.parametrize('case', SHIFTED, ids=lambda c: c.id)
def test_wide_walk_agrees_with_the_wide_shift(case):
    """
    The first block of the case's circuit, its first row.  Every rotation is exp(-i theta sigma / 2) between fixed linear maps, so
    with the pattern held fixed d f / d theta = (f(theta + pi/2) - f(theta - pi/2)) / 2 exactly (f: the value of the sampled
    family, the unnormalised numerator of the jump family).  Tolerance, with eps = 2^-63, h = max|h'| and K the operations of the
    block (one per rotation, CNOT, Pauli and relaxation site):
      * an operation rewrites an amplitude as a sum of two complex products, 4 roundings relative to a state of norm at most 1;
        three chains of K operations meet in the comparison (psi and lambda in the walk, psi in the shifted forward): 12 K eps h;
      * the read-out and an inner product add D terms each: 2 D eps h;  the shifted angle is rounded once, |theta| + pi/2 < 5;
      * the jump family divides by the N2 of the unshifted walk, and no state's norm exceeds 1: the whole over min N2.
    n >= 10: every fifth angle (the walk's entries are compared where the shift is evaluated).
    """
    cfgs, x, w, ro = _first_block(case)
    n, D = case.n, 1 << case.n
    i = TP.inputs_of(case)
    real = np.longdouble
    step = 5 if n >= 10 else 1
    if case.family == 'sampled':
        v, gx, gw = NTG.traj_grad(n, cfgs, x, w, i.noise, row0=case.row0, dtype=TP.WIDE, **ro)
        weights = NTG.readout_weights(n, ro['offset'], ro['coeff'], ro['ham_diag'], float(i.noise.readout), real)
        f = lambda xx, ww: NO.replay_values(n, cfgs, xx, ww, i.noise, ro['offset'], ro['coeff'], ro['ham_diag'], ro['ham_pauli'],
                                            case.row0, TP.WIDE, weights).mean(axis=1)
        floor, h = 1.0, float(np.abs(weights[1]).max())
    else:
        r = G.walk(n, cfgs, x, w, i.nz, TP.T, case.seed, row0=case.row0, dtype=TP.WIDE, **ro)
        gx, gw = r['gx'], r['gw']
        f = lambda xx, ww: G.walk(n, cfgs, xx, ww, i.nz, TP.T, case.seed, row0=case.row0, forced=r['pattern'], grad=False,
                                  dtype=TP.WIDE, **ro)['num'] / r['N2']
        floor = float(r['N2'].min())
        h = float(np.abs(DT.readout_weights(n, ro['offset'], ro['coeff'], ro['ham_diag'], i.nz['readout01'], i.nz['readout10'])[1]).max())
    K = n * (2 + 8 * cfgs[0][1])                                             # per wire: RX, its site; per sub-layer 3 rotations,
    tol = EPS * h * (12 * K + 2 * D + 5) / floor                             # a CNOT, 4 sites (ROT, TGT, CTL and a Pauli)
    hp = NTG.half_pi(real)
    xw, ww = x.astype(real), w.astype(real)
    worst = 0.0
    for e in range(0, x.shape[1], step):
        d = np.zeros_like(xw)
        d[:, e] = hp
        worst = max(worst, float(np.abs((f(xw + d, ww) - f(xw - d, ww)) / 2 - gx[:, e]).max()))
    for idx in list(np.ndindex(w.shape))[::step]:
        d = np.zeros_like(ww)
        d[idx] = hp
        worst = max(worst, float(np.abs((f(xw, ww + d) - f(xw, ww - d)) / 2 - gw[(slice(None),) + idx]).max()))
    peak = float(max(np.abs(gx).max(), np.abs(gw).max()))
    print(f'{case.id}: max|walk - shift| {worst:.2e}  tolerance {tol:.2e} ({K} operations, h {h:.2f}, min N2 {floor:.2e})  max|g| {peak:.2e}')
    assert gx.dtype == np.longdouble and worst <= tol
    assert tol < 2.0 ** -53 * 8 * h and peak > 1e-3 * h                      # finer than fp64 could tell, and not vacuous


# ---------------------------------------------------------------------------------------------------------------------
# the finding
# ---------------------------------------------------------------------------------------------------------------------
def test_inverse_walk_without_restart_leaves_the_budget_past_12():
    """jump-q7-10x2-past12 as planned (traj_precision_cases.LOWERED; gamma = 1 - exp(-12.8 / t1) on 490 sites, LEVEL 12.05): what
    the kernels compute -- K0^-1 through every site that did not fire -- is wrong in every digit in fp64 numpy, while the
    stored walk and the inverse walk that restores psi at 10^RESTART_TABLED are inside the budget the rule gives with the
    restarted walk as its second reference.  Figures of numpy here: without a restart 4.7e+4 on a largest entry of 61, with it
    1.5e-12, the stored walk's own error."""
    case = TP.past12_q7()
    assert case.id in TP.LOWERED and case.id not in IDS
    ld = {q: TP.split(v) for q, v in TP.quantities(*TP.walk(case, 'stored', dtype=TP.WIDE)).items()}
    forms = {'no restart': TP.quantities(*TP.walk(case, 'inverse', restart_above=None)),
             'stored': TP.quantities(*TP.walk(case, 'stored')),
             'restart': TP.quantities(*TP.walk(case, 'inverse', restart_above=G.RESTART_TABLED))}
    assert float(TP.pattern_walk(case)['level'].max()) > 12.0
    for q in TP.QUANTITIES:
        e = {k: TP._maxabs(err(v[q], ld[q])) for k, v in forms.items()}
        peak = TP._maxabs(ld[q][0])
        bud = TP.FACTOR * max(e['stored'], e['restart'], TP.ULP * peak)
        print(f'{case.id} {q}: {e}  budget {bud:.2e}  max|q| {peak:.2e}')
        assert e['stored'] <= bud and e['restart'] <= bud
        if q == 'row':
            assert bud <= 2.0 ** -10 * peak and e['no restart'] > bud and e['no restart'] > peak
    # one decade up the restart comes too late (the table of DESIGN.md 7p)
    late = TP.quantities(*TP.walk(case, 'inverse', restart_above=G.RESTART_TABLED + 1.0))
    assert TP._maxabs(err(late['row'], ld['row'])) > TP._maxabs(ld['row'][0])


def test_python_layer_refuses_what_the_table_does_not_support():
    """quanonet_amd.noise.JUMP_GAMMA_MAX: the lowered past-12 setting is refused by the call and by the solver's key before
    anything is launched; every case that runs with all wires alike (hot = 0) lies below the bound; gamma = 1 keeps its message"""
    import torch
    from quanonet_amd import noise as N
    from quanonet_amd.solver import DataParallelTrainer, FlatAdam
    case = TP.past12_q7()
    i = TP.inputs_of(case)
    gamma, site, wire = N.jump_gamma_max(i.noise, case.n)
    assert gamma > N.JUMP_GAMMA_MAX and gamma == DT.jump_pairs(case.n, i.nz)[..., 0].max()
    with pytest.raises(ValueError, match='JUMP_GAMMA_MAX'):
        N.device_trajectory_loss_and_grad(i.model, i.ins, torch.zeros(1), i.noise, i.sampling)
    with pytest.raises(ValueError, match='JUMP_GAMMA_MAX'):
        N.device_sampled_loss_and_grad(i.model, i.ins, torch.zeros(1), i.noise, i.sampling)
    # the solver's key: DataParallelTrainer._jump_loss itself, on the attributes it reads (its checks come before any launch)
    trainer = SimpleNamespace(sampling_key='train_jump_trajectories', desc=i.model.fused_desc(), optimizer=object.__new__(FlatAdam),
                              train_device_noise=i.noise)
    with pytest.raises(ValueError, match='train_device_noise with train_jump_trajectories.*JUMP_GAMMA_MAX'):
        DataParallelTrainer._jump_loss(trainer, None)
    for c in JUMP:
        if not c.hot:
            assert N.jump_gamma_max(TP.inputs_of(c).noise, c.n)[0] <= N.JUMP_GAMMA_MAX, c.id
            N.check_jump_gradient_setting(TP.inputs_of(c).noise, c.n, c.id)
    dead = N.DeviceNoise(t1=1e-3, t2=1e-3, t_rx=0.1, t_rot=0.1, t_cx=0.1)
    N.check_jump_gradient_setting(dead, 7, 'dead')                            # gamma = 1: the C call's own refusal
