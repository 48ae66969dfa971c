"""
Members with n = 10..12 (workgroup-resident kernels, hea_lds.hip) in the member entry points: ensembles, sweeps, depth sweeps and
qubit sweeps train them in the same launches as their other members -- lds_bwd_kernel<N, DepthArgs / QubitArgs>, one launch per
n present and step -- instead of one single-model call per member.

* the number of kernels a call launches does not grow with the member count (stream capture, graph never instantiated);
* every member's parameters, Adam moments and [grads | sse | sum y^2] rows are BITWISE those of model_train_steps on that
  member alone, row tails untouched;
* members match the CPU oracle + torch.optim.Adam at 1e-10, and QubitSweepSolver matches the PTSolver runs of its configs.
"""
import os

import numpy as np
import pytest
import torch

from tests.test_ensemble import _antideriv, _data, _flat, _heaqnn, _oracle_adam, _quanonet, _run_single, _schedule
from tests.test_depth_sweep import _run_depth
from tests.test_qubit_sweep import SENTINEL, _run_qubit
from tests.helpers import assert_checkpoints_bitwise, kernels_launched as _kernels_launched, member_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ensemble_call(dev, models, inputs, ys, bounds, gbs, lr, ham_diag=None):
    """(call, outputs): the ensemble call on fresh tensors, rows wider than P + 2 (SENTINEL tails)"""
    return member_call(dev, 'ensemble', models, [lr] * len(models), inputs, ys, bounds, gbs, ham_diag=ham_diag,
                       rows_sentinel=SENTINEL, rows_extra=3)


def _sweep_call(dev, models, lrs, inputs, ys, bounds, gbs, ham_diag=None):
    return member_call(dev, 'sweep', models, lrs, inputs, ys, bounds, gbs, ham_diag=ham_diag, rows_sentinel=SENTINEL,
                       rows_extra=3)


def _qubit_call(dev, models, lrs, inputs, ys, bounds, gbs):
    return member_call(dev, 'qubit', models, lrs, inputs, ys, bounds, gbs)[0]


def test_q10_ensemble_launches_do_not_grow_with_r(dev):
    net = (1, 1, 2, 1)
    bounds, gbs = _schedule(32, 2)
    counts = {}
    for R in (2, 4):
        inputs, ys = _data(R, bounds[-1], (4, 2), 3000 + R)
        models = [_quanonet(10, 4, 2, net, s, scale_coeff=0.1, if_trainable_freq=True) for s in range(R)]
        call, _ = _ensemble_call(dev, models, inputs, ys, bounds, gbs, 1e-3)
        counts[R] = _kernels_launched(dev, call)
    assert counts[2] == counts[4], counts
    assert counts[2] <= 1 + 3 * len(gbs), counts          # member records, then prep, backward, reduce per step


def test_qubit_sweep_one_backward_launch_per_n_present(dev):
    cells = [(3, (2, 1, 1, 1)), (10, (1, 1, 2, 1)), (10, (2, 1, 1, 1)), (11, (1, 1, 1, 1))]
    bounds, gbs = _schedule(32, 2)
    inputs, ys = _data(len(cells), bounds[-1], (4, 2), 3100)
    models = [_quanonet(n, 4, 2, net, i, scale_coeff=0.1, if_trainable_freq=True) for i, (n, net) in enumerate(cells)]
    call = _qubit_call(dev, models, [1e-3] * len(cells), inputs, ys, bounds, gbs)
    k = _kernels_launched(dev, call)
    # member records and work lists once per call; per step one prep, one backward launch per register class or n present
    # (n = 3..6 class, n = 10, n = 11) and one reduce
    assert k <= 2 + len(gbs) * (1 + 3 + 1), k


# ---- bitwise: every member equals its single-model run ----
def _check_bitwise(dev, models, lrs, got, inputs, ys, bounds, gbs, ham_diag=None):
    params, m_, v_, rows = (t.cpu() for t in got)
    for i, model in enumerate(models):
        P = _flat(model).numel()
        hd = None if ham_diag is None else torch.from_numpy(np.asarray(ham_diag[i], np.float64)).to(dev)
        want = _run_single(dev, model.fused_desc(), model, inputs[i], ys[i], bounds, gbs, lrs[i], ham_diag=hd)
        for g, w, what in zip((params, m_, v_), want[:3], ('params', 'exp_avg', 'exp_avg_sq')):
            assert torch.equal(g[i], w), (i, what, float((g[i] - w).abs().max()))
        assert torch.equal(rows[i, :, :P + 2], want[3]), (i, 'rows', float((rows[i, :, :P + 2] - want[3]).abs().max()))
        assert bool((rows[i, :, P + 2:] == SENTINEL).all()), (i, 'gradient row tail written')


@pytest.mark.parametrize('variant', ['auto', 'packed'])
def test_q10_seed_ensemble_bitwise(dev, variant):
    from quanonet_amd import _lib
    net = (2, 1, 2, 1)
    bounds, gbs = _schedule(64, 3, last=29)
    inputs, ys = _data(3, bounds[-1], (4, 2), 3200)
    models = [_quanonet(10, 4, 2, net, s, scale_coeff=0.1, if_trainable_freq=True) for s in range(3)]
    _lib.set_backward_variant(variant)
    try:
        call, got = _ensemble_call(dev, models, inputs, ys, bounds, gbs, 2e-3)
        call()
        _lib.check_status(dev)
        _check_bitwise(dev, models, [2e-3] * 3, got, inputs, ys, bounds, gbs)
    finally:
        _lib.set_backward_variant('auto')


@pytest.mark.parametrize('variant', ['auto', 'packed'])
def test_q10_sweep_mixed_readout_lr_and_ham_diag_bitwise(dev, variant):
    from quanonet_amd import _lib
    net = (1, 2, 2, 1)
    bounds, gbs = _schedule(48, 2)
    _lib.set_backward_variant(variant)
    try:
        # X / Z read-outs with their own Hamiltonian bounds, learning rate per member
        inputs, ys = _data(3, bounds[-1], (4, 2), 3300)
        models = [_quanonet(10, 4, 2, net, i, scale_coeff=0.1, if_trainable_freq=True, ham_pauli='XZX'[i],
                            ham_bound=(-1.0 - i, 2.0)) for i in range(3)]
        lrs = [1e-3, 3e-3, 5e-4]
        call, got = _sweep_call(dev, models, lrs, inputs, ys, bounds, gbs)
        call()
        _lib.check_status(dev)
        _check_bitwise(dev, models, lrs, got, inputs, ys, bounds, gbs)
        # a diagonal Hamiltonian of 2^10 entries per member
        rng = np.random.default_rng(3301)
        inputs, ys = _data(2, bounds[-1], (4, 2), 3302)
        models = [_quanonet(10, 4, 2, net, 10 + i, scale_coeff=0.1, if_trainable_freq=True,
                            ham_diag=np.sort(rng.uniform(-3, 3, size=1 << 10))) for i in range(2)]
        hd = [m.quantum_layer.ham_diag.detach().cpu().numpy().astype(np.float64) for m in models]
        assert [len(h) for h in hd] == [1024, 1024]
        call, got = _sweep_call(dev, models, [1e-3, 2e-3], inputs, ys, bounds, gbs, ham_diag=hd)
        call()
        _lib.check_status(dev)
        _check_bitwise(dev, models, [1e-3, 2e-3], got, inputs, ys, bounds, gbs, ham_diag=hd)
    finally:
        _lib.set_backward_variant('auto')


@pytest.mark.parametrize('variant', ['auto', 'packed'])
def test_n11_depth_sweep_fixed_frequency_short_last_batch_bitwise(dev, variant):
    from quanonet_amd import _lib
    nets = [(1, 1, 2, 1), (2, 1, 1, 1), (1, 1, 1, 1)]
    bounds, gbs = _schedule(40, 3, last=17)
    inputs, ys = _data(len(nets), bounds[-1], (4, 2), 3400)
    models = [_quanonet(11, 4, 2, net, i, scale_coeff=0.2, if_trainable_freq=False) for i, net in enumerate(nets)]
    lrs = [1e-3, 2e-3, 4e-3]
    _lib.set_backward_variant(variant)
    try:
        got = _run_depth(dev, models, lrs, inputs, ys, bounds, gbs)
        for i, model in enumerate(models):
            P = _flat(model).numel()
            want = _run_single(dev, model.fused_desc(), model, inputs[i], ys[i], bounds, gbs, lrs[i])
            for g, w, what in zip(got[:3], want[:3], ('params', 'exp_avg', 'exp_avg_sq')):
                assert torch.equal(g[i, :P], w), (i, what, float((g[i, :P] - w).abs().max()))
                assert bool((g[i, P:] == SENTINEL).all()), (i, what, 'row tail written')
            assert torch.equal(got[3][i, :, :P + 2], want[3]), (i, 'rows')
    finally:
        _lib.set_backward_variant('auto')


def _qubit_bitwise(dev, models, lrs, inputs, ys, bounds, gbs):
    from quanonet_amd import _lib
    _lib.set_backward_variant('packed')
    try:
        got = _run_qubit(dev, models, lrs, inputs, ys, bounds, gbs)
        for i, model in enumerate(models):
            P = _flat(model).numel()
            want = _run_single(dev, model.fused_desc(), model, inputs[i], ys[i], bounds, gbs, lrs[i])
            for g, w, what in zip(got[:3], want[:3], ('params', 'exp_avg', 'exp_avg_sq')):
                assert torch.equal(g[i, :P], w), (i, what, float((g[i, :P] - w).abs().max()))
                assert bool((g[i, P:] == SENTINEL).all()), (i, what, 'row tail written')
            assert torch.equal(got[3][i, :, :P + 2], want[3]), (i, 'rows', float((got[3][i, :, :P + 2] - want[3]).abs().max()))
            assert bool((got[3][i, :, P + 2:] == SENTINEL).all()), (i, 'gradient row tail written')
    finally:
        _lib.set_backward_variant('auto')


def test_qubit_sweep_with_n10_and_n12_members_bitwise(dev):
    cells = [(2, (3, 1, 2, 1)), (5, (2, 1, 1, 1)), (10, (1, 1, 2, 1)), (10, (2, 1, 1, 1)), (12, (1, 1, 1, 1))]
    bounds, gbs = _schedule(24, 2, last=13)
    inputs, ys = _data(len(cells), bounds[-1], (4, 2), 3500)
    models = [_quanonet(n, 4, 2, net, i, scale_coeff=0.1, if_trainable_freq=True) for i, (n, net) in enumerate(cells)]
    _qubit_bitwise(dev, models, [1e-3, 2e-3, 5e-4, 1e-3, 3e-3], inputs, ys, bounds, gbs)


def test_heaqnn_qubit_sweep_with_n10_and_n12_members_bitwise(dev):
    cells = [(2, (2, 2)), (5, (3, 2)), (10, (2, 2)), (10, (1, 2)), (12, (1, 2))]          # (the linear depth is shared)
    bounds, gbs = _schedule(24, 2, last=11)
    inputs, ys = _data(len(cells), bounds[-1], (4,), 3600)
    models = [_heaqnn(n, 4, net, i) for i, (n, net) in enumerate(cells)]
    _qubit_bitwise(dev, models, [1e-3] * len(cells), inputs, ys, bounds, gbs)


# ---- the oracle and the solver ----
def test_n10_sweep_members_match_the_oracle(dev):
    from oracle import hea_oracle as O
    from oracle import c_oracle as C
    net = (1, 1, 2, 1)
    bounds, gbs = _schedule(32, 2, last=20)
    inputs, ys = _data(2, bounds[-1], (4, 2), 3700)
    models = [_quanonet(10, 4, 2, net, i, scale_coeff=0.1, if_trainable_freq=True) for i in range(2)]
    lrs = [1e-3, 2e-3]
    call, got = _sweep_call(dev, models, lrs, inputs, ys, bounds, gbs)
    call()
    from quanonet_amd import _lib
    _lib.check_status(dev)
    got_p, got_rows = got[0].cpu(), got[3].cpu()

    def lg(sd, ins, y, gb):
        loss, grads, _ = O.quanonet_loss_and_grads(sd, ins[0], ins[1], y, 10, net, ham_bound=(-5.0, 5.0), batch_total=gb,
                                                   engine=C)
        return loss, grads
    for i, model in enumerate(models):
        want_rows, want_p = _oracle_adam(model, lg, inputs[i], ys[i], bounds, gbs, lrs[i])
        P = want_p.size
        err_r = np.abs(got_rows[i][:, :P + 2].numpy() - want_rows).max() / max(1.0, np.abs(want_rows).max())
        err_p = np.abs(got_p[i].numpy() - want_p).max() / max(1.0, np.abs(want_p).max())
        assert err_r < 1e-10 and err_p < 1e-10, (i, err_r, err_p)


BASE = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'scale_coeff': 0.001, 'if_trainable_freq': 'true',
        'learning_rate': 1e-3, 'batch_size': 100, 'num_epochs': 2}


@pytest.mark.parametrize('variant', ['auto', 'packed'])
def test_q2_q10_qubit_sweep_solver_matches_ptsolver_runs(dev, tmp_path, variant):
    from quanonet_amd import _lib
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    from quanonet_amd.solver import PTSolver, set_random_seed
    cfgs = [dict(BASE, seed=s, num_qubits=n, net_size=[hb, 2, ht, 2], run_id=f'q{n}_hb{hb}_ht{ht}_s{s}')
            for (n, hb, ht, s) in ((2, 5, 5, 0), (10, 1, 2, 0), (10, 2, 1, 1))]
    data = _antideriv(450)
    quiet = lambda *a, **k: None
    _lib.set_backward_variant(variant)
    try:
        sw = QubitSweepSolver([dict(c, prefix=str(tmp_path / 'sweep')) for c in cfgs], data, device=dev, log=quiet)
        hists = sw.train()
        metrics = sw.evaluate(hists)
        for c, h, mt, m in zip(cfgs, hists, metrics, sw.members):
            set_random_seed(c['seed'])
            solo = PTSolver(dict(c, prefix=str(tmp_path / 'solo')), data, device=dev, log=quiet)
            hs = solo.train()
            ms = solo.evaluate(hs)
            p_sw, p_solo = m.trainer.pflat.cpu(), solo.trainer.pflat.cpu()
            exact = variant == 'packed' or c['num_qubits'] >= 10     # (n >= 10: one kernel whatever the variant)
            if exact:
                assert torch.equal(p_sw, p_solo), c
                assert h['loss_train'] == hs['loss_train'], c
                assert mt['rel_l2'] == ms['rel_l2'], c
                assert_checkpoints_bitwise(m.out_dir, solo.out_dir, c)
            else:
                assert float((p_sw - p_solo).abs().max()) < 1e-10, c
                assert np.allclose(h['loss_train'], hs['loss_train'], rtol=1e-10, atol=0), c
                assert np.isclose(mt['rel_l2'], ms['rel_l2'], rtol=1e-10, atol=0), c
            for f in ('best_model.pt', 'final.pt'):
                a = torch.load(os.path.join(m.out_dir, f))
                b = torch.load(os.path.join(solo.out_dir, f))
                assert a.keys() == b.keys()
                for k in a:
                    if exact:
                        assert torch.equal(a[k], b[k]), (c, f, k)
                    else:
                        assert float((a[k] - b[k]).abs().max()) < 1e-10, (c, f, k)
    finally:
        _lib.set_backward_variant('auto')
