"""
Runs of training steps whose reduce kernel writes the next step's layer records (``qhea_model_train_steps`` on
block-unrolled shapes), at bench.py's model and at the batches around it.

In that reduce kernel each gate's half-angle sincos and ZYZ decomposition run in the lanes that have just updated the
gate's angles, and the frequency blocks load their Adam state with the column sums.  Here K = 6 steps of one
``train_steps`` call are compared with:

* the same steps one ``train_step`` call at a time, whose records come from a prep launch per step: every step's
  ``[grads | sse | sum y^2]`` row, the parameters and both Adam moments bitwise equal;
* an independent CPU loop, oracle gradients (C engine) + ``torch.optim.Adam``, at the tolerance of
  tests/test_benched_path.py.

The n = 2, one-sub-layer shape puts two circuit blocks in one reduce block: the other layout of the records' gates.
"""
import copy

import numpy as np
import pytest
import torch

from tests.helpers import oracle_adam_loop

pytestmark = pytest.mark.gpu
TOL = 1e-9
STEPS = 6


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _model(n, b_in, net, seed):
    from quanonet_amd.models import QuanONetPT
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = QuanONetPT(n, b_in, 2, net, scale_coeff=0.1, if_trainable_freq=True).double()
    with torch.no_grad():                           # non-trivial frequency biases (the init is zeros)
        model.branch_freq.bias.copy_(torch.from_numpy(rng.normal(scale=0.3, size=model.branch_freq.bias.shape)))
        model.trunk_freq.bias.copy_(torch.from_numpy(rng.normal(scale=0.3, size=model.trunk_freq.bias.shape)))
        model.bias.fill_(0.2)
    return model


@pytest.mark.parametrize('n,b_in,net,batch', [
    (5, 100, (40, 2, 20, 2), 1024),      # bench.py's workload
    (5, 100, (40, 2, 20, 2), 512),
    (5, 100, (40, 2, 20, 2), 100),
    (2, 7, (5, 1, 5, 1), 64),            # two circuit blocks per reduce block
])
def test_fused_record_steps_equal_single_steps_and_oracle(dev, n, b_in, net, batch):
    from quanonet_amd.solver import DataParallelTrainer
    lr = 1e-3                                       # larger than the bench's 1e-4: the steps must differ visibly
    rng = np.random.default_rng(1000 + batch + n)
    n_rows = STEPS * batch - batch // 3             # uneven last batch
    branch = rng.normal(size=(n_rows, b_in)); trunk = rng.uniform(size=(n_rows, 2))
    y = rng.normal(scale=0.5, size=n_rows)
    bounds = list(range(0, n_rows, batch)) + [n_rows]
    gbs = [bounds[i + 1] - bounds[i] for i in range(len(bounds) - 1)]
    assert len(gbs) == STEPS

    model = _model(n, b_in, net, seed=batch + n)
    cpu_model = copy.deepcopy(model)
    names = [k for k, _ in cpu_model.named_parameters()]
    want_rows, want_params = oracle_adam_loop(cpu_model, names, branch, trunk, y, bounds, gbs, n, net, lr)

    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    br, tk, yy = t(branch), t(trunk), t(y).reshape(-1, 1)
    many = DataParallelTrainer(copy.deepcopy(model).to(dev), lr=lr)
    single = DataParallelTrainer(copy.deepcopy(model).to(dev), lr=lr)
    assert many.accepts_out and torch.equal(many.pflat, single.pflat)
    rows_m = torch.zeros(STEPS, many.numel + 2, dtype=torch.float64, device=dev)
    rows_s = torch.zeros_like(rows_m)
    many.train_steps([br, tk], yy, bounds, gbs, rows_m)
    for i in range(STEPS):
        lo, hi = bounds[i], bounds[i + 1]
        single.train_step(br[lo:hi], tk[lo:hi], yy[lo:hi], global_batch=gbs[i], out=rows_s[i])
    torch.cuda.synchronize()
    many.check_status(); single.check_status()

    assert torch.equal(rows_m, rows_s)
    assert torch.equal(many.pflat, single.pflat)
    assert torch.equal(many.optimizer.exp_avg, single.optimizer.exp_avg)
    assert torch.equal(many.optimizer.exp_avg_sq, single.optimizer.exp_avg_sq)
    assert many.optimizer.t == single.optimizer.t == STEPS

    got = rows_m.cpu().numpy()
    for i in range(STEPS):
        np.testing.assert_allclose(got[i], want_rows[i], rtol=0, atol=TOL, err_msg=f'step {i}')
    np.testing.assert_allclose(many.pflat.cpu().numpy(), want_params, rtol=0, atol=TOL)
    assert np.abs(want_rows[0][:-2] - want_rows[-1][:-2]).max() > 1e-6      # the steps moved the parameters
