"""
The references and the case table of the exact noisy forwards' error budgets (tests/forward_precision_cases.py).  CPU only.

* the table: every (kernel, N) from 2 to 9 has a case, every family each read-out letter, the n <= 6 cases one row more than a
  workgroup of the launcher holds, the per-wire device setting no two wires or slots alike;
* the references of every case: the two fp64 evaluations agree with q_ld to 1e-12, the second form's probabilities (uniform
  family: the Kraus form; device family: the stored forward) equal the channel form's, the sequential read-out equals the
  pairwise one to 1e-13, q_ld carries more than 53 bits;
* the condition on the inputs that keeps a budget from being vacuous: budget(pred) <= 1e-12 and budget(sd) <= 1e-12 on every
  case, two orders below the atol the functional tests hold these kernels to; from the references alone, printed per case.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import device_noise_reference as DNR
from tests import forward_precision_cases as FP
from tests import helpers as H
from tests.conftest import ROOT

IDS = [c.id for c in FP.CASES]


@pytest.fixture(scope='module')
def lib():
    """(a model's constructor loads the library)"""
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_table():
    assert len(set(IDS)) == len(IDS)
    assert [FP.row_slots(n) for n in (2, 3, 4, 5, 6)] == [256, 64, 16, 4, 1]         # the launcher's text was read as it is meant
    by = lambda fam: [c for c in FP.CASES if c.family == fam]
    assert {c.n for c in by('uniform')} == {c.n for c in by('device')} == {2, 3, 4, 5, 6}
    assert {c.n for c in by('wide')} == {7, 8, 9}
    for fam in ('uniform', 'device', 'wide'):
        assert {c.readout for c in by(fam)} == {'Z', 'X', 'Y', 'diag'}, fam
        assert any(c.kind == 'quanonet' for c in by(fam)), fam
    for c in FP.CASES:
        assert c.rows == ((1 if c.n == 9 else 2) if c.family == 'wide' else FP.row_slots(c.n) + 1)
        assert (c.noise in FP.NOISES) == (c.family != 'device')
        assert c.rows <= 300
    for fam in ('uniform', 'wide'):
        for n in {c.n for c in by(fam)}:
            assert {c.noise for c in by(fam) if c.n == n and c.net == (3, 2)} >= set(FP.NOISES), (fam, n)
    assert {(c.n, c.net) for c in by('uniform')} >= {(5, (60, 2)), (6, (10, 2)), (3, (2, 0))}
    assert {(c.n, c.net, c.noise) for c in by('device')} >= {(5, (8, 2), 'calibration'), (5, (3, 2), 'calibration')}
    assert any(c.noise == 'perwire-noidle' for c in by('device'))
    # the edges of the wide unit nothing else compares with a reference
    assert {(c.kind, c.net) for c in by('wide') if c.n == 8} >= {('heaqnn', (2, 0)), ('quanonet', (2, 0, 1, 2))}
    assert {c.readout for c in by('wide') if c.n == 9 and c.noise != 'none'} >= {'X', 'Y'}
    for key, (was, now, why) in FP.LOWERED.items():
        assert was == (60, 2) and now[0] < was[0] and now[1] == was[1] and why
        assert key not in IDS and key.replace(f'{was[0]}x{was[1]}', f'{now[0]}x{now[1]}') in IDS
    assert 'uniform-q5-60x2-none' in IDS                                 # the trained depth itself, gates only
    # the unnamed namespace in a kernel's mangled name, one and two template arguments
    name = '_ZN4qhea12_GLOBAL__N_118density_fwd_kernelILi5EEEvNS0_8DensArgsE'
    assert FP._is(H.mangled_is, name, 'density_fwd_kernel', (5,)) and not FP._is(H.mangled_is, name, 'density_fwd_kernel', (6,))
    assert not FP._is(H.mangled_is, name, 'density_dev_fwd_kernel')
    assert not FP._is(H.mangled_is, name.replace('18density_fwd', '22density_dev_fwd'), 'density_fwd_kernel')
    ring = '_ZN4qhea12_GLOBAL__N_124density_wide_ring_kernelILi7ELi1EEEvNS0_8DensArgsEP15HIP_vector_typeIdLj2EEiiii'
    assert FP._is(H.mangled_is, ring, 'density_wide_ring_kernel', (7,)) and not FP._is(H.mangled_is, ring, 'density_wide_ring_kernel', (9,))
    assert not FP._is(H.mangled_is, ring, 'density_wide_wires_kernel')


@pytest.mark.parametrize('n', [2, 3, 4, 6])
def test_perwire_setting_has_no_two_wires_alike(n):
    from tests.test_device_noise_training_abi import as_dict
    for idle in (True, False):
        d = as_dict(FP.perwire_setting(n, idle), n)
        for key in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2'):
            assert len(set(d[key])) == n, (key, d[key])
        assert all(a != b for a, b in zip(d['readout01'], d['readout10'])) and d['idle'] is idle


def test_kernel_readout_is_the_confusion_matrix():
    """the two-point mixes of the value table against the 2^n x 2^n confusion matrix written out, asymmetric flips"""
    n, D = 3, 8
    rng = np.random.default_rng(0)
    r01, r10 = [0.01, 0.2, 0.05], [0.3, 0.02, 0.07]
    hv = rng.normal(size=D)
    prob = rng.dirichlet(np.ones(D), size=4)
    conf = np.ones((D, D))                                               # conf[read, true]
    for read in range(D):
        for true in range(D):
            for i in range(n):
                rb, tb = (read >> i) & 1, (true >> i) & 1
                conf[read, true] *= (r01[i] if rb else 1 - r01[i]) if tb == 0 else (r10[i] if rb == 0 else 1 - r10[i])
    m1, m2 = FP.kernel_readout(prob, n, r01, r10, hv)
    pread = prob @ conf.T
    np.testing.assert_allclose(m1, pread @ hv, rtol=0, atol=1e-15)
    np.testing.assert_allclose(m2, pread @ (hv * hv), rtol=0, atol=1e-15)


@pytest.mark.parametrize('cid', ['uniform-q3-3x2-heavy-X', 'uniform-q4-3x2-readme-Y', 'device-q3-3x2-perwire-X', 'device-q4-3x2-perwire-Y'])
def test_probabilities_are_the_references_own(lib, cid):
    """forward_precision_cases evolves to the Z basis and changes the basis afterwards (cases that differ in the read-out alone
    share the evolution): bit for bit what the references' final_rho returns for the read-out"""
    from tests import density_grad_reference as DG
    from tests import density_reference as DR
    from tests import device_noise_grad_reference as DV
    case = next(c for c in FP.CASES if c.id == cid)
    i = FP.inputs_of(case)
    mc = DG.model_circuit(i.spec, i.flat, i.branch, i.trunk)
    nz, pauli = FP.noise_dict(case), i.spec['ham_pauli']
    if case.family == 'uniform':
        channel = DR.final_rho(mc.n, mc.cfgs, mc.x, mc.w, i.noise.p1, i.noise.p2, pauli)
        second = DNR.final_rho(mc.n, mc.cfgs, mc.x, mc.w, nz, pauli)
    else:
        channel = DNR.final_rho(mc.n, mc.cfgs, mc.x, mc.w, nz, pauli)
        second = DV.stored_final_rho(mc.n, mc.cfgs, mc.x, mc.w, nz, pauli)
    for form, rho in (('channel', channel), ('second', second)):
        assert np.array_equal(FP.probabilities(case, form)[0], np.real(np.einsum('bkk->bk', rho))), form
    for a, b in FP.SHARED.items():
        ia, ib = (FP.inputs_of(next(c for c in FP.CASES if c.id == k)) for k in (a, b))
        assert np.array_equal(ia.flat, ib.flat) and np.array_equal(ia.branch, ib.branch) and ia.noise == ib.noise
        assert ia.spec['ham_pauli'] != ib.spec['ham_pauli'] == 'Z'


@pytest.mark.parametrize('case', FP.CASES, ids=IDS)
def test_references_and_the_condition_on_the_inputs(lib, case):
    ref = FP.reference(case)
    for q in FP.QUANTITIES:
        hi, lo = ref.ld[q]
        print(f'{case.id} {q}: e_ref {FP.e_ref(ref, q):.2e} (channel form {ref.e_c[q]:.2e}, second form {ref.e_np[q]:.2e})  '
              f'budget {FP.budget(ref, q):.2e}  scale {FP.scale(ref, q):.2e}  min|q| {np.abs(hi).min():.2e}  max|q| {FP._maxabs(hi):.2e}')
        assert hi.shape == (case.rows,) and np.isfinite(hi).all() and np.isfinite(lo).all()
        assert (np.abs(lo) <= np.spacing(np.abs(hi))).all(), q               # lo is what hi leaves over: the reference was wide
        assert ref.e_c[q] <= 1e-12 and ref.e_np[q] <= 1e-12, (q, ref.e_c[q], ref.e_np[q])
        assert FP.scale(ref, q) > 0.25
        # not vacuous: two orders below the atol = 1e-10 of the functional tests
        assert FP.budget(ref, q) <= FP.CAP, (q, FP.budget(ref, q))
        assert FP.budget(ref, q) == FP.FACTOR * max(FP.e_ref(ref, q), FP.ULP * FP.scale(ref, q))
    assert FP._maxabs(ref.ld['pred'][1]) > 0.0 and (ref.ld['sd'][0] > 0.1).all()
    # the second form is the same state and the same read-out in other arithmetic
    p_channel, _ = FP.probabilities(case, 'channel')
    p_second, _ = FP.probabilities(case, 'second')
    assert FP._maxabs(p_channel - p_second) <= 1e-13
    s, nz = ref.inputs.spec, FP.noise_dict(case)
    m1, m2 = FP.kernel_readout(p_second, case.n, nz['readout01'], nz['readout10'],
                               DNR.value_table(case.n, s['offset'], s['coeff'], s['ham_diag']))
    mean, var = FP.pairwise_moments(case, p_second)
    print(f'{case.id}: sequential - pairwise read-out  m1 {FP._maxabs(m1 - mean):.2e}  var {FP._maxabs(m2 - m1 * m1 - var):.2e}')
    assert FP._maxabs(m1 - mean) <= 1e-13 and FP._maxabs(m2 - m1 * m1 - var) <= 1e-13
