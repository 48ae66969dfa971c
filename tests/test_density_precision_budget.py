"""
Error budgets of the density-matrix gradient kernels on the device: density_bwd_kernel<N>, density_dev_bwd_kernel<N> and
density_dev_stored_bwd_kernel<N> against the helper's stored walk in extended precision, from log10 A = 0 to their guards at
the depths that are trained; each quantity within budget(q) = 32 x max(e_ref(q), 2^-53 max|q|), e_ref the error of the two fp64
numpy walks (stored and inverse) on the same inputs (tests/density_precision_cases.py: the table and the rule;
tests/test_density_precision_oracle.py: the references and the condition that keeps the budgets from being vacuous).

Each case makes its one loss_grad call, asserts by name the kernel and the N that ran, asserts everything finite and then
max|got - q_ld| <= budget(q) for the gradient row, the sse and pred.  The atol = 1e-10 the other noisy-gradient tests use is
larger than the whole gradient at the guard (largest entry 9.5e-12 .. 1.6e-10 at log10 A = 11.99) and up to 0.4 % of it at
log10 A = 8; these budgets are at most 2^-10 of the largest gradient entry, by the condition the CPU file puts on the inputs.
Measured figures: profiles/r35_density_precision_budget.json, DESIGN.md section 4.
"""
import numpy as np
import pytest
import torch

from tests import density_precision_cases as DP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.mark.parametrize('case', DP.CASES, ids=lambda c: c.id)
def test_density_gradient_kernels_stay_within_their_error_budget(dev, case):
    ref = DP.reference(case)
    got, kernel = DP.run_case(dev, case)
    for q in DP.QUANTITIES:
        assert np.isfinite(got[q]).all(), (case.id, q)
    failures = []
    for q in DP.QUANTITIES:
        error, e_ref, budget = DP.measure(got, ref, q)
        ratio = error / e_ref if e_ref else float('inf') if error else 0.0
        print(f'{case.id} {q}: error {error:.2e}  e_ref {e_ref:.2e}  ratio {ratio:.1f}  budget {budget:.2e}  '
              f'max|q| {DP._maxabs(ref.ld[q][0]):.2e}')
        if not error <= budget:
            failures.append(f'{q}: error {error:.3e} > budget {budget:.3e} (e_ref {e_ref:.3e}, error / e_ref {ratio:.1f})')
    assert not failures, f'{case.id} {kernel}: ' + '; '.join(failures)
