"""
Error budgets on the device: every kernel family against the long-double oracle, each quantity within
budget(q) = 32 x max(e_ref(q), 2^-53 max|q|), e_ref the two fp64 oracles' own error on the same inputs
(tests/precision_cases.py: the table, the rule and why 32; tests/test_precision_oracle.py: the references).

Each case runs under its variant, asserts by name the kernels it launched, asserts everything finite and then
max|got - q_ld| <= budget(q) per quantity: out, state, grad_x, grad_w and the backward's own out at circuit level; the
gradient row, the sse and the predictions of one qhea_model_loss_grad call at model level.
"""
import numpy as np
import pytest
import torch

from tests import precision_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _assert_within_budget(case, got, ref, kernels, quantities):
    for q, ld_q in quantities:
        assert np.isfinite(got[q]).all(), (case.id, q)
    failures = []
    for q, ld_q in quantities:
        err, e_ref, budget = PC.measure(got, ref, q, ld_q)
        print(f'{case.id} {q}: error {err:.2e}  e_ref {e_ref:.2e}  ratio {err / e_ref:.1f}  budget {budget:.2e}')
        if not err <= budget:
            failures.append(f'{q}: error {err:.3e} > budget {budget:.3e} (e_ref {e_ref:.3e}, error / e_ref {err / e_ref:.1f})')
    assert not failures, f'{case.id} {kernels}: ' + '; '.join(failures)


@pytest.mark.parametrize('case', PC.CIRCUIT_CASES, ids=lambda c: c.id)
def test_circuit_kernels_stay_within_their_error_budget(dev, cus, case):
    ref = PC.circuit_reference(case, case.batch(cus))
    got, kernels = PC.run_circuit_case(dev, case, cus)
    _assert_within_budget(case, got, ref, kernels, [('out', 'out'), ('state', 'state'), ('grad_x', 'grad_x'),
                                                    ('grad_w', 'grad_w'), ('backward out', 'out')])


@pytest.mark.parametrize('case', PC.MODEL_CASES, ids=lambda c: c.id)
def test_model_loss_grad_stays_within_its_error_budget(dev, cus, case):
    ref = PC.model_reference(case)
    got, kernels = PC.run_model_case(dev, case, cus)
    _assert_within_budget(case, got, ref, kernels, [('row', 'row'), ('sse', 'sse'), ('out', 'out')])
