"""
The extended-precision stored walk and the case table of the density-matrix gradient budgets (tests/density_precision_cases.py).
CPU only.

* threading a dtype through the numpy helpers changed no fp64 result: one small case per helper (and per forward), bit for bit
  against values the helpers gave before they took a dtype (tests/golden/density_helper_fp64_pins.npz);
* the wide stored walk reproduces the fp64 stored walk to 1e-12 on every case, and on the n = 2 and n = 3 cases, cut to their
  first block, it agrees with parameter shift through the wide forward to a tolerance made of the wide type's epsilon and the
  operation count;
* every case's log10 A / A_dev is within 1e-6 of its target and inside the guard of the call it makes (the past-the-guard
  stored case: the inverse call's guard refuses it);
* the condition on the inputs that keeps a budget from being vacuous: budget(row) <= 2^-10 max|row_ld| on every case.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import density_grad_reference as DG
from tests import density_precision_cases as DP
from tests import density_reference as DR
from tests import device_noise_grad_reference as DV
from tests import device_noise_reference as DNR
from tests import helpers as H
from tests.conftest import ROOT

IDS = [c.id for c in DP.CASES]
EPS = float(np.finfo(np.longdouble).eps)             # 2^-63 on x86


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_table():
    assert len(set(IDS)) == len(IDS)
    assert np.finfo(np.longdouble).nmant >= 63
    by = lambda fam: [c for c in DP.CASES if c.family == fam]
    assert {(c.n, c.net, c.target) for c in by('stored')} == {(5, (30, 2), 7.0), (3, (30, 2), 7.0), (3, (6, 2), 16.0)}
    assert {c.n for c in by('uniform')} == {c.n for c in by('device')} == {2, 3, 4, 5, 6}
    for c in DP.CASES:
        assert c.rows == (3 if c.kind == 'quanonet' else 1 if c.n >= 5 else 2)
        rpw = max(1, 64 >> (2 * c.n - 4))                                # launch_density_bwd: row slots of a workgroup
        assert c.n >= 5 or (1 < c.rows and c.rows % rpw != 0)            # more than one slot filled, a tail slot left
        assert c.readout == {3: 'X', 4: 'Y'}.get(c.n, 'diag' if (c.n, c.net, c.target) == (5, (30, 2), 8.0) else 'Z') or c.past
    for key, (was, now, why) in DP.LOWERED.items():
        assert now in (10.0, 8.0) and now < was and why
        assert key not in IDS and key.replace(f'A{was:g}', f'A{now:g}') in IDS
    # the unnamed namespace in a kernel's mangled name
    name = '_ZN4qhea12_GLOBAL__N_118density_bwd_kernelILi5EEEvNS0_12DensGradArgsE'
    assert DP._is(H.mangled_is, name, 'density_bwd_kernel', (5,)) and not DP._is(H.mangled_is, name, 'density_bwd_kernel', (6,))
    assert not DP._is(H.mangled_is, name, 'density_dev_bwd_kernel')
    assert not DP._is(H.mangled_is, name.replace('18density_bwd', '22density_dev_bwd'), 'density_bwd_kernel')


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 helpers are bit for bit what they were
# ---------------------------------------------------------------------------------------------------------------------
def test_fp64_helpers_are_bitwise_unchanged():
    """tests/golden/density_helper_fp64_pins.npz holds the inputs and what the four routines returned before `dtype` existed
    (durations chosen so that numpy's exp gives the same bits with and without its AVX-512 kernels)"""
    g = np.load(os.path.join(H.GOLDEN, 'density_helper_fp64_pins.npz'))
    t_rx, t_rot, t_cx = (float(v) for v in g['durations'])
    spec_u = dict(kind='heaqnn', n=3, net=(2, 2), trainable=True, scale=None, offset=0.5, coeff=5.0 / 6.0, ham_diag=None,
                  ham_pauli='Y')
    spec_d = dict(kind='quanonet', n=2, net=(1, 1, 1, 2), trainable=False, scale=0.7, offset=0.0, coeff=1.0,
                  ham_diag=g['device_diag'], ham_pauli='Z')
    nz2 = dict(p1=[0.02, 0.03], p2=[0.05, 0.04], readout01=[0.01, 0.02], readout10=[0.03, 0.04], t1=[1.0, float('inf')],
               t2=[1.5, 4.0], t_rx=t_rx, t_rot=t_rot, t_cx=t_cx, idle=True)
    for inverse in (False, True):
        buf, pred = DG.model_loss_grad(spec_u, g['uniform_flat'], g['uniform_x'], None, g['uniform_y'], 0.03, 0.08, 0.04, 1.0 / 7,
                                       inverse=inverse)
        assert buf.dtype == np.float64 and pred.dtype == np.float64
        assert np.array_equal(buf, g[f'uniform_grad_{int(inverse)}']) and np.array_equal(pred, g[f'uniform_pred_{int(inverse)}'])
        buf, pred = DV.model_loss_grad(spec_d, g['device_flat'], g['device_branch'], g['device_trunk'], g['device_y'], nz2, 1.0 / 5,
                                       inverse=inverse)
        assert buf.dtype == np.float64 and pred.dtype == np.float64
        assert np.array_equal(buf, g[f'device_grad_{int(inverse)}']) and np.array_equal(pred, g[f'device_pred_{int(inverse)}'])
    cfgs = [(3, 1), (3, 0), (3, 2)]
    nz3 = dict(p1=[0.02, 0.03, 0.01], p2=[0.05, 0.04, 0.06], readout01=[0.01, 0.02, 0.01], readout10=[0.03, 0.04, 0.02],
               t1=[1.0, float('inf'), 1.5], t2=[1.5, 4.0, 1.0], t_rx=t_rx, t_rot=t_rot, t_cx=t_cx, idle=False)
    x, w = g['forward_x'], g['forward_w']
    assert np.array_equal(np.stack(DR.exact_moments(3, cfgs, x, w, 0.03, 0.08, 0.04, offset=0.3, coeff=1.7, ham_pauli='X')),
                          g['forward_uniform'])
    assert np.array_equal(np.stack(DNR.device_moments(3, cfgs, x, w, nz3, offset=0.3, coeff=1.7, ham_pauli='Y')), g['forward_device'])
    # and the wide walk is the same function: it differs from the pins by fp64 rounding only, in a wide array
    buf, _ = DG.model_loss_grad(spec_u, g['uniform_flat'], g['uniform_x'], None, g['uniform_y'], 0.03, 0.08, 0.04, 1.0 / 7, dtype=DP.WIDE)
    assert buf.dtype == np.longdouble and 0 < np.abs(buf - g['uniform_grad_0']).max() < 1e-13
    buf, _ = DV.model_loss_grad(spec_d, g['device_flat'], g['device_branch'], g['device_trunk'], g['device_y'], nz2, 1.0 / 5, dtype=DP.WIDE)
    assert buf.dtype == np.longdouble and 0 < np.abs(buf - g['device_grad_0']).max() < 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', DP.CASES, ids=IDS)
def test_references_and_the_condition_on_the_inputs(case):
    ref = DP.reference(case)
    for q in DP.QUANTITIES:
        hi, lo = ref.ld[q]
        peak = DP._maxabs(hi)
        print(f'{case.id} {q}: e_ref {DP.e_ref(ref, q):.2e} (stored walk {ref.e_c[q]:.2e}, inverse walk {ref.e_np[q]:.2e})  '
              f'budget {DP.budget(ref, q):.2e}  max|q| {peak:.2e}  budget / max|q| {DP.budget(ref, q) / peak:.2e}')
        assert np.isfinite(hi).all() and np.isfinite(lo).all()
        assert (np.abs(lo) <= np.spacing(np.abs(hi))).all(), q                # lo is what hi leaves over: the walk was wide
        assert ref.e_c[q] <= 1e-12, (q, ref.e_c[q])                           # the wide stored walk is the fp64 stored walk
    # the residuals do not cancel (density_precision_cases.SEEDS): the row is not made of pred's last bits
    pred, y = ref.ld['pred'][0], np.asarray(ref.inputs.y)
    assert (np.abs(pred - y) >= np.abs(pred) / 8).all(), (pred, y)
    # not vacuous: the budget resolves at least three digits of the largest gradient entry
    assert DP.budget(ref, 'row') <= 2.0 ** -10 * DP._maxabs(ref.ld['row'][0])
    assert DP._maxabs(ref.ld['row'][1]) > 0.0                                 # ... and the reference carries more than 53 bits


@pytest.mark.parametrize('case', DP.CASES, ids=IDS)
def test_targets_and_guards(lib, case):
    from quanonet_amd.noise import amplification, device_amplification, device_layer_amplification
    from tests.test_device_noise_training_abi import _loss_grad, as_dict
    i = DP.inputs_of(case)
    assert abs(i.logA - case.target) < 1e-6, (i.logA, case.target)
    if case.rates:
        assert abs(case.target - 3.3) < 0.05                                  # the README's figure for these rates
    if case.family == 'uniform':
        assert abs(DG.log10_amplification(case.n, DP.cfgs_of(case), i.noise.p1, i.noise.p2) - i.logA) < 1e-12
        assert amplification(i.model, i.noise) <= DP.GUARD['uniform']
        return
    assert abs(DV.log10_amplification(case.n, DP.cfgs_of(case), as_dict(i.noise, case.n)) - i.logA) < 1e-12
    total = device_amplification(i.model, i.noise)
    assert abs(total - i.logA) < 1e-9
    rec = i.noise.params(case.n)
    if case.family == 'stored':
        assert device_layer_amplification(i.model, i.noise) <= DP.GUARD['stored']
    if case.past:
        assert total > DP.GUARD['device'] and _loss_grad(lib, i.model.fused_desc(), 0, rec) == -2      # the inverse call refuses
    else:
        assert total <= DP.GUARD['device'] and _loss_grad(lib, i.model.fused_desc(), 0, rec) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the wide stored walk against parameter shift through the wide forward
# ---------------------------------------------------------------------------------------------------------------------
def _first_block(case):
    """(cfgs, x, w, read-out kwargs) of the case's circuit cut to its first block, in float64"""
    i = DP.inputs_of(case)
    assert case.kind == 'heaqnn' and not i.spec['trainable']
    n, ld = case.n, case.net[1]
    x = DG._tiled(i.branch, n) * i.spec['scale']
    w = i.flat.reshape(-1, 3, n)[:ld]
    kw = dict(offset=i.spec['offset'], coeff=i.spec['coeff'], ham_diag=i.spec['ham_diag'], ham_pauli=i.spec['ham_pauli'])
    return [(n, ld)], x, w, kw


@pytest.mark.parametrize('case', [c for c in DP.CASES if c.n <= 3], ids=lambda c: c.id)
def test_wide_walk_agrees_with_parameter_shift_through_the_wide_forward(case):
    """
    Every rotation is exp(-i theta sigma / 2) between linear maps, so d f / d theta = (f(theta + pi/2) - f(theta - pi/2)) / 2
    exactly.  Tolerance, with eps = 2^-63 and h = max|h'| (|f| <= h and |d f / d theta| <= h):
      * a gate or a channel rewrites an element of rho (or O) as a sum of two products on the row side and two on the column
        side: 4 roundings, each relative to a magnitude of at most 1 (h for O).  K operations in the circuit, three chains of
        them in the comparison -- rho and O in the walk, rho in the shifted forward --: 3 K * 4 eps h;
      * the traces Tr(O sigma rho) and sum_k p_k h'_k add D^2 and D terms: (D^2 + D) eps h;
      * the shifted angle theta +- pi/2 is rounded once, |theta| + pi/2 < 5: 5 eps h.
    """
    from tests.test_device_noise_training_abi import as_dict
    real = np.longdouble
    cfgs, x, w, kw = _first_block(case)
    n, D = case.n, 1 << case.n
    i = DP.inputs_of(case)
    half_pi = 2 * np.arctan(real(1))
    if case.family == 'uniform':
        p = (i.noise.p1, i.noise.p2, i.noise.readout)
        v, gx, gw = DG.circuit_grad(n, cfgs, x, w, *p, dtype=DP.WIDE, **kw)
        f = lambda xx, ww: DR.exact_moments(n, cfgs, xx, ww, *p, dtype=DP.WIDE, **kw)[0]
        K = len(DG._ops(n, cfgs))
        h = float(np.abs(DG.value_table(n, p[2], kw['offset'], kw['coeff'], kw['ham_diag'])).max())
    else:
        nz = as_dict(i.noise, n)
        v, gx, gw = DV.circuit_grad(n, cfgs, x, w, nz, dtype=DP.WIDE, **kw)
        f = lambda xx, ww: DNR.device_moments(n, cfgs, xx, ww, nz, dtype=DP.WIDE, **kw)[0]
        K = len(DV._ops(n, cfgs, nz))
        h = float(np.abs(DV.value_table(n, nz, kw['offset'], kw['coeff'], kw['ham_diag'])).max())
    tol = EPS * h * (3 * K * 4 + D * D + D + 5)
    xw, ww = x.astype(real), w.astype(real)
    worst = float(np.abs(f(xw, ww) - v).max())
    for e in range(x.shape[1]):
        d = np.zeros_like(xw)
        d[:, e] = half_pi
        worst = max(worst, float(np.abs((f(xw + d, ww) - f(xw - d, ww)) / 2 - gx[:, e]).max()))
    for idx in np.ndindex(w.shape):
        d = np.zeros_like(ww)
        d[idx] = half_pi
        worst = max(worst, float(np.abs((f(xw, ww + d) - f(xw, ww - d)) / 2 - gw[(slice(None),) + idx]).max()))
    peak = float(max(np.abs(gx).max(), np.abs(gw).max()))
    print(f'{case.id}: max|walk - shift| {worst:.2e}  tolerance {tol:.2e} ({K} operations, h {h:.2f})  max|g| {peak:.2e}')
    assert gx.dtype == np.longdouble and worst <= tol
    assert tol < 2.0 ** -53 * 8 and peak > 1e-3 * h                          # finer than fp64 could tell, and not vacuous
