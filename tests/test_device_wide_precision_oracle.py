"""
The references and the case table of the error budgets of the exact forward under a device noise model at n = 7..9
(tests/device_wide_precision_cases.py).  CPU only; the checks are those tests/test_forward_precision_oracle.py makes of its table.

* the table: n = 7, 8, 9 at (3, 2) with the per-wire setting, one case without the idle decay, an X read-out at n = 9, an
  encoding-only (2, 0) case; the per-wire setting has no two wires or slots alike at these sizes either;
* the references of every case: the two fp64 evaluations agree with q_ld to 1e-12, the stored forward's probabilities equal the
  Kraus timeline's, the sequential read-out equals the pairwise one to 1e-13, q_ld carries more than 53 bits;
* the condition on the inputs that keeps a budget from being vacuous: budget(pred) <= 1e-12 and budget(sd) <= 1e-12 on every
  case, from the references alone, printed per case.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import device_noise_reference as DNR
from tests import device_wide_precision_cases as DW
from tests import forward_precision_cases as FP
from tests.conftest import ROOT

IDS = [c.id for c in DW.CASES]


@pytest.fixture(scope='module')
def lib():
    """(a model's constructor loads the library)"""
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_table():
    assert len(set(IDS)) == len(IDS) and not set(IDS) & {c.id for c in FP.CASES}
    assert {(c.n, c.net, c.noise) for c in DW.CASES} >= {(n, (3, 2), 'perwire') for n in (7, 8, 9)}
    assert any(c.noise == 'perwire-noidle' for c in DW.CASES)
    assert any(c.n == 9 and c.readout == 'X' for c in DW.CASES) and any(c.net == (2, 0) for c in DW.CASES)
    for c in DW.CASES:
        assert c.family == 'device' and c.rows == (1 if c.n == 9 else 2) and c.noise in ('perwire', 'perwire-noidle')
    for a, b in DW.SHARED.items():
        ia, ib = (DW.inputs_of(next(c for c in DW.CASES if c.id == k)) for k in (a, b))
        assert np.array_equal(ia.flat, ib.flat) and np.array_equal(ia.branch, ib.branch) and ia.noise == ib.noise
        assert ia.spec['ham_pauli'] != ib.spec['ham_pauli'] == 'Z'
    assert not DW.LOWERED and DW.CAP == 1e-12
    ring = '_ZN4qhea12_GLOBAL__N_128density_dev_wide_ring_kernelILi7ELi1EEEvNS0_12DevStageArgsEP15HIP_vector_typeIdLj2EEiiii'
    from tests.density_precision_cases import _is
    from tests.helpers import mangled_is
    assert _is(mangled_is, ring, DW.KERNELS[0], (7,)) and not _is(mangled_is, ring, DW.KERNELS[0], (9,))
    assert not _is(mangled_is, ring, FP.WIDE_KERNELS[0]) and not _is(mangled_is, ring, DW.KERNELS[1])


@pytest.mark.parametrize('n', [7, 8, 9])
def test_perwire_setting_has_no_two_wires_alike(n):
    from tests.test_device_noise_training_abi import as_dict
    for idle in (True, False):
        d = as_dict(DW.perwire_setting(n, idle), n)
        for key in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2'):
            assert len(set(d[key])) == n, (key, d[key])
        assert all(a != b for a, b in zip(d['readout01'], d['readout10'])) and d['idle'] is idle
        if n != 8:
            assert DW.perwire_setting(n, idle) == FP.perwire_setting(n, idle)


@pytest.mark.parametrize('case', DW.CASES, ids=IDS)
def test_references_and_the_condition_on_the_inputs(lib, case):
    ref = DW.reference_of(case)
    for q in DW.QUANTITIES:
        hi, lo = ref.ld[q]
        print(f'{case.id} {q}: e_ref {FP.e_ref(ref, q):.2e} (channel form {ref.e_c[q]:.2e}, second form {ref.e_np[q]:.2e})  '
              f'budget {DW.budget(ref, q):.2e}  scale {DW.scale(ref, q):.2e}  min|q| {np.abs(hi).min():.2e}  max|q| {FP._maxabs(hi):.2e}')
        assert hi.shape == (case.rows,) and np.isfinite(hi).all() and np.isfinite(lo).all()
        assert (np.abs(lo) <= np.spacing(np.abs(hi))).all(), q               # lo is what hi leaves over: the reference was wide
        assert ref.e_c[q] <= 1e-12 and ref.e_np[q] <= 1e-12, (q, ref.e_c[q], ref.e_np[q])
        assert DW.scale(ref, q) > 0.25
        # not vacuous: two orders below the atol = 1e-10 of the functional tests
        assert DW.budget(ref, q) <= DW.CAP, (q, DW.budget(ref, q))
        assert DW.budget(ref, q) == FP.FACTOR * max(FP.e_ref(ref, q), FP.ULP * DW.scale(ref, q))
    assert FP._maxabs(ref.ld['pred'][1]) > 0.0 and (ref.ld['sd'][0] > 0.1).all()
    # the second form is the same state and the same read-out in other arithmetic
    p_channel, _ = DW.probabilities(case, 'channel')
    p_second, _ = DW.probabilities(case, 'second')
    assert FP._maxabs(p_channel - p_second) <= 1e-13
    s, nz = ref.inputs.spec, FP.noise_dict(case)
    m1, m2 = FP.kernel_readout(p_second, case.n, nz['readout01'], nz['readout10'],
                               DNR.value_table(case.n, s['offset'], s['coeff'], s['ham_diag']))
    mean, var = FP.pairwise_moments(case, p_second)
    print(f'{case.id}: sequential - pairwise read-out  m1 {FP._maxabs(m1 - mean):.2e}  var {FP._maxabs(m2 - m1 * m1 - var):.2e}')
    assert FP._maxabs(m1 - mean) <= 1e-13 and FP._maxabs(m2 - m1 * m1 - var) <= 1e-13
