"""
Error budgets of the exact noisy forward kernels on the device: density_fwd_kernel<N> and density_dev_fwd_kernel<N> for N = 2..6
and the tiled chain of hea_density_wide.hip for N = 7, 8, 9 against the channel-form reference in extended precision; pred and
shot_std each within budget(q) = 32 x max(e_ref(q), 2^-53 scale(q)), e_ref the error of two fp64 numpy evaluations of other
arithmetic on the same inputs (tests/forward_precision_cases.py: the table and the rule; tests/test_forward_precision_oracle.py:
the references and the condition that keeps the budgets from being vacuous).

Each case makes its one forward call, asserts by name the kernels and the N that ran, asserts everything finite and sd >= 0 and
then max|got - q_ld| <= budget(q).  The atol = 1e-10 the functional tests hold these kernels to is four orders above their
error; these budgets are at most 1e-12, by the condition the CPU file puts on the inputs.
Measured figures: profiles/r38_forward_precision_budget.json, DESIGN.md section 4.
"""
import numpy as np
import pytest
import torch

from tests import forward_precision_cases as FP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.mark.parametrize('case', FP.CASES, ids=lambda c: c.id)
def test_exact_noisy_forward_kernels_stay_within_their_error_budget(dev, case):
    ref = FP.reference(case)
    got, kernels = FP.run_case(dev, case)
    for q in FP.QUANTITIES:
        assert got[q].shape == (case.rows,) and np.isfinite(got[q]).all(), (case.id, q)
    assert (got['sd'] >= 0.0).all()
    failures = []
    for q in FP.QUANTITIES:
        error, e_ref, budget = FP.measure(got, ref, q)
        ratio = error / e_ref if e_ref else float('inf') if error else 0.0
        print(f'{case.id} {q}: error {error:.2e}  e_ref {e_ref:.2e}  ratio {ratio:.1f}  budget {budget:.2e}  '
              f'scale {FP.scale(ref, q):.2e}')
        if not error <= budget:
            failures.append(f'{q}: error {error:.3e} > budget {budget:.3e} (e_ref {e_ref:.3e}, error / e_ref {ratio:.1f})')
    assert not failures, f'{case.id} {kernels}: ' + '; '.join(failures)
