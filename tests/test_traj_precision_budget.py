"""
Error budgets of the sampled-Pauli and the quantum-jump trajectory gradient kernels on the GPU (tests/traj_precision_cases.py):
every case, every quantity of one loss_grad call inside 32 x max(e_ref, 2^-53 max|q|) against the extended-precision walk, the launched
kernel asserted by name and by its template argument n.  Prints error / e_ref per case.
"""
import pytest
import torch

from tests import traj_precision_cases as TP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.mark.parametrize('case', TP.CASES, ids=[c.id for c in TP.CASES])
def test_inside_the_budget(dev, case):
    ref = TP.reference(case)
    got, kernel = TP.run_case(dev, case)
    figures = {q: TP.measure(got, ref, q) for q in TP.QUANTITIES}
    for q, (e, e_ref, bud) in figures.items():
        print(f'{case.id} {q}: error {e:.2e}  e_ref {e_ref:.2e}  error / e_ref {e / max(e_ref, 1e-300):.2f}  budget {bud:.2e}  '
              f'error / budget {e / bud:.3f}  [{kernel}]')
    for q, (e, e_ref, bud) in figures.items():
        assert e <= bud, (case.id, q, e, bud)
