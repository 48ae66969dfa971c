"""
Error budgets of the exact forward under a device noise model at n = 7, 8, 9 on the device: the kernel chain of
hea_density_device_wide.hip against the Kraus timeline in extended precision; pred and shot_std each within
budget(q) = 32 x max(e_ref(q), 2^-53 scale(q)) (tests/device_wide_precision_cases.py: the table; tests/forward_precision_cases.py:
the rule and the references; tests/test_device_wide_precision_oracle.py: the condition that keeps the budgets from being
vacuous, budget <= 1e-12).

Each case makes its one forward call, asserts by name the kernels and the N that ran, asserts everything finite and sd >= 0 and
then max|got - q_ld| <= budget(q).
"""
import numpy as np
import pytest
import torch

from tests import device_wide_precision_cases as DW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.mark.parametrize('case', DW.CASES, ids=lambda c: c.id)
def test_device_wide_kernels_stay_within_their_error_budget(dev, case):
    ref = DW.reference_of(case)
    got, kernels = DW.run_case(dev, case)
    for q in DW.QUANTITIES:
        assert got[q].shape == (case.rows,) and np.isfinite(got[q]).all(), (case.id, q)
    assert (got['sd'] >= 0.0).all()
    failures = []
    for q in DW.QUANTITIES:
        error, e_ref, budget = DW.measure(got, ref, q)
        ratio = error / e_ref if e_ref else float('inf') if error else 0.0
        print(f'{case.id} {q}: error {error:.2e}  e_ref {e_ref:.2e}  ratio {ratio:.1f}  budget {budget:.2e}  '
              f'scale {DW.scale(ref, q):.2e}')
        if not error <= budget:
            failures.append(f'{q}: error {error:.3e} > budget {budget:.3e} (e_ref {e_ref:.3e}, error / e_ref {ratio:.1f})')
    assert not failures, f'{case.id} {kernels}: ' + '; '.join(failures)
