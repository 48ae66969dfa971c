"""
The snapshot pipeline (QHEA_BWD_ZSNAP, ``bwd_zsnap_kernel``): psi taken from the forward sweep's snapshots at every
publication point, lambda walked back in the split layout, two sample groups per workgroup.

* the headline model (cfg 2) at 513 ... 1024 samples, ragged batches included (a last group with one sample, a last
  workgroup with one group), three training steps against the oracle + ``torch.optim.Adam`` at 1e-9;
* random block-unrolled n = 5 shapes against the oracle with the variant forced;
* against ``ztri2`` (psi walked back): parameters agree to 1e-12 relative after several steps;
* two identical runs are bitwise equal, and a multi-step ``train_steps`` call equals the same steps as single calls;
* with the spin-bound-1 library (child process): an overrun is reported (NaN gradients, no Adam update, -6), then clean.
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from oracle import c_oracle as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_QUBITS, NET, B_IN, T_IN = 5, (40, 2, 20, 2), 100, 2


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _headline_model(rng, seed=0):
    from quanonet_amd.models import QuanONetPT
    torch.manual_seed(seed)
    model = QuanONetPT(N_QUBITS, B_IN, T_IN, NET, scale_coeff=0.1, if_trainable_freq=True).double()
    with torch.no_grad():
        model.branch_freq.bias.copy_(torch.from_numpy(rng.normal(scale=0.3, size=model.branch_freq.bias.shape)))
        model.trunk_freq.bias.copy_(torch.from_numpy(rng.normal(scale=0.3, size=model.trunk_freq.bias.shape)))
        model.bias.fill_(0.2)
    return model


def _train(model, dev, variant, branch, trunk, y, bounds, gbs, lr):
    """train_steps on a copy of `model` with `variant` forced: (rows [steps, P+2], final flat parameters)."""
    from quanonet_amd import _lib
    from quanonet_amd.solver import DataParallelTrainer
    _lib.set_backward_variant(variant)
    try:
        tr = DataParallelTrainer(copy.deepcopy(model).to(dev), lr=lr)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        rows = torch.zeros(len(gbs), tr.numel + 2, dtype=torch.float64, device=dev)
        tr.train_steps([t(branch), t(trunk)], t(y).reshape(-1, 1), bounds, gbs, rows)
        torch.cuda.synchronize()
        tr.check_status()
    finally:
        _lib.set_backward_variant('auto')
    return rows.cpu().numpy(), tr.pflat.cpu().numpy()


def _oracle_adam(model, branch, trunk, y, bounds, gbs, n, net, lr, scale_coeff=None):
    cpu = copy.deepcopy(model)
    names = [k for k, _ in cpu.named_parameters()]
    params = [p for _, p in cpu.named_parameters()]
    opt = torch.optim.Adam(params, lr=lr)
    rows = []
    for i in range(len(gbs)):
        lo, hi = bounds[i], bounds[i + 1]
        sd = {k: v.detach().numpy() for k, v in cpu.state_dict().items()}
        loss, grads, _ = O.quanonet_loss_and_grads(sd, branch[lo:hi], trunk[lo:hi], y[lo:hi], n, net,
                                                   batch_total=gbs[i], scale_coeff=scale_coeff, engine=C)
        flat = np.concatenate([np.asarray(grads[k], np.float64).reshape(-1) for k in names])
        rows.append(np.concatenate([flat, [loss * gbs[i], float((y[lo:hi] ** 2).sum())]]))
        opt.zero_grad()
        for k, p in zip(names, params):
            p.grad = torch.from_numpy(np.asarray(grads[k], np.float64).reshape(p.shape).copy())
        opt.step()
    return np.stack(rows), np.concatenate([p.detach().numpy().reshape(-1) for p in params])


def _data(rng, n_rows, b_in=B_IN, t_in=T_IN):
    return rng.normal(size=(n_rows, b_in)), rng.uniform(size=(n_rows, t_in)), rng.normal(scale=0.5, size=n_rows)


@pytest.mark.parametrize('batch', [1024, 1000, 768, 600, 520, 513])
def test_headline_steps_match_oracle_and_torch_adam(dev, batch):
    steps, lr = 3, 1e-3
    rng = np.random.default_rng(500 + batch)
    branch, trunk, y = _data(rng, steps * batch)
    bounds = [i * batch for i in range(steps + 1)]
    gbs = [batch] * steps
    model = _headline_model(rng)
    want_rows, want_params = _oracle_adam(model, branch, trunk, y, bounds, gbs, N_QUBITS, NET, lr)
    for variant in ('zsnap', 'auto'):
        got_rows, got_params = _train(model, dev, variant, branch, trunk, y, bounds, gbs, lr)
        for i in range(steps):
            np.testing.assert_allclose(got_rows[i], want_rows[i], rtol=0, atol=1e-9, err_msg=f'{variant} step {i}')
        np.testing.assert_allclose(got_params, want_params, rtol=0, atol=1e-9, err_msg=variant)
    assert np.abs(want_rows[0][:-2] - want_rows[2][:-2]).max() > 1e-6


def test_random_block_unrolled_shapes_match_oracle(dev):
    from quanonet_amd.models import QuanONetPT
    rng = np.random.default_rng(11)
    for case in range(12):
        ld = int(rng.integers(1, 3))
        net = (int(rng.integers(1, 6)), ld, int(rng.integers(1, 6)), ld)
        B = int(rng.choice([1, 3, 64, 129, 513, 700, 1024]))
        b_in, t_in = int(rng.integers(2, 9)), int(rng.integers(1, 3))
        torch.manual_seed(case)
        tf = bool(case % 3)
        model = QuanONetPT(5, b_in, t_in, net, scale_coeff=0.3, if_trainable_freq=tf).double()
        with torch.no_grad():
            for k, p in model.named_parameters():
                if 'freq' in k and 'bias' in k:
                    p.copy_(torch.from_numpy(rng.normal(scale=0.3, size=p.shape)))
        branch, trunk, y = _data(rng, 2 * B, b_in, t_in)
        bounds, gbs = [0, B, 2 * B], [B, B]
        want_rows, want_params = _oracle_adam(model, branch, trunk, y, bounds, gbs, 5, net, 1e-2, None if tf else 0.3)
        got_rows, got_params = _train(model, dev, 'zsnap', branch, trunk, y, bounds, gbs, 1e-2)
        err = np.abs(got_rows - want_rows).max()
        assert err < 1e-9, (case, net, B, err)
        assert np.abs(got_params - want_params).max() < 1e-9, (case, net, B)


@pytest.mark.parametrize('batch', [1024, 777])
def test_agrees_with_psi_walked_back(dev, batch):
    steps, lr = 6, 1e-3
    rng = np.random.default_rng(900 + batch)
    branch, trunk, y = _data(rng, steps * batch)
    bounds = [i * batch for i in range(steps + 1)]
    model = _headline_model(rng, seed=1)
    _, p_snap = _train(model, dev, 'zsnap', branch, trunk, y, bounds, [batch] * steps, lr)
    _, p_tri = _train(model, dev, 'ztri2', branch, trunk, y, bounds, [batch] * steps, lr)
    rel = np.abs(p_snap - p_tri) / np.maximum(np.abs(p_tri), 1e-300)
    assert np.abs(p_snap - p_tri).max() <= 1e-12 * np.abs(p_tri).max(), rel.max()
    assert np.allclose(p_snap, p_tri, rtol=1e-12, atol=1e-15)


def test_bitwise_reproducible_and_multi_step_equals_single_steps(dev):
    steps, batch, lr = 4, 1024, 1e-3
    rng = np.random.default_rng(4)
    branch, trunk, y = _data(rng, steps * batch)
    bounds = [i * batch for i in range(steps + 1)]
    model = _headline_model(rng, seed=2)
    rows_a, p_a = _train(model, dev, 'zsnap', branch, trunk, y, bounds, [batch] * steps, lr)
    rows_b, p_b = _train(model, dev, 'zsnap', branch, trunk, y, bounds, [batch] * steps, lr)
    assert np.array_equal(rows_a, rows_b) and np.array_equal(p_a, p_b)

    from quanonet_amd import _lib
    from quanonet_amd.solver import DataParallelTrainer
    _lib.set_backward_variant('zsnap')
    try:
        tr = DataParallelTrainer(copy.deepcopy(model).to(dev), lr=lr)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        single = []
        for i in range(steps):
            rows = torch.zeros(tr.numel + 2, dtype=torch.float64, device=dev)
            sl = slice(i * batch, (i + 1) * batch)
            tr.train_step(t(branch[sl]), t(trunk[sl]), t(y[sl]), global_batch=batch, out=rows)
            single.append(rows.cpu().numpy())
        torch.cuda.synchronize()
        tr.check_status()
    finally:
        _lib.set_backward_variant('auto')
    assert np.array_equal(np.stack(single), rows_a) and np.array_equal(tr.pflat.cpu().numpy(), p_a)


SPIN1 = os.path.join(ROOT, 'quanonet_amd', 'libquanonet_hea_spin1.so')
CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from quanonet_amd import _lib
from quanonet_amd.models import QuanONetPT
from quanonet_amd.solver import DataParallelTrainer
assert _lib.LIB_PATH.endswith('libquanonet_hea_spin1.so'), _lib.LIB_PATH
dev = torch.device('cuda:0')
torch.manual_seed(0)
rng = np.random.default_rng(0)
model = QuanONetPT(5, 8, 2, (3, 2, 2, 2), scale_coeff=0.1, if_trainable_freq=True).to(dev)
tr = DataParallelTrainer(model, lr=1e-2, fused=True)
_lib.set_backward_variant('zsnap')
for B in (64, 1024):
    br = torch.tensor(rng.normal(size=(B, 8)), device=dev); tk = torch.tensor(rng.uniform(size=(B, 2)), device=dev)
    y = torch.tensor(rng.normal(size=B), device=dev)
    before = tr.pflat.clone()
    flat = tr.train_step(br, tk, y).clone()
    torch.cuda.synchronize()
    assert torch.isnan(flat[:tr.numel]).all(), (B, 'gradients must be NaN-poisoned')
    assert torch.isnan(flat[tr.numel]), (B, 'sse must be NaN')
    assert torch.equal(tr.pflat, before), (B, 'the fused Adam update must be skipped')
    try:
        tr.check_status()
        raise SystemExit(f'{B}: check_status did not raise')
    except _lib.QheaError as e:
        assert '(-6)' in str(e), str(e)
    tr.check_status()                                           # reading the status clears it
    tr.optimizer.t = 0
print('ZSNAP_STATUS_OK')
'''


def test_overrun_is_reported_under_zsnap():
    assert os.path.exists(SPIN1), "build it with `make -C quanonet_amd/csrc spin1` (__graft_entry__.build() does)"
    env = dict(os.environ, QHEA_LIB=SPIN1)
    r = subprocess.run([sys.executable, '-c', CHILD % {'root': ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'ZSNAP_STATUS_OK' in r.stdout, r.stdout + r.stderr
