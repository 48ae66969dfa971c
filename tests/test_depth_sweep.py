"""
Depth sweep on the GPU (qhea_model_depth_sweep_train_steps, quanonet_amd.depth_sweep.DepthSweepSolver): R models whose circuit
depths differ (and read-out, scale, learning rate), every step of all members as one launch per kernel.

* every member's parameters, Adam moments and [grads | sse | sum y^2] rows are BITWISE those of model_train_steps on that member
  alone under the packed backward variant -- Q2 with ZYZ-eligible and ineligible depths, Q3, Q6, fixed frequency, mixed X / Z
  read-out, ham_diag spectra, HEAQNN, a short last batch; the rows' tails beyond each member's vector stay untouched;
* the members match the CPU oracle + torch.optim.Adam at 1e-10; an n = 10 grid (one member after the other) gives each member's
  single-model result;
* DepthSweepSolver matches the PTSolver runs its configs describe, checkpoints and evaluate metrics included.
"""
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_checkpoints_bitwise, run_members
from tests.test_ensemble import _data, _flat, _heaqnn, _oracle_adam, _quanonet, _run_single, _schedule

pytestmark = pytest.mark.gpu
SENTINEL = 12345.678


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _run_depth(dev, models, lrs, inputs, ys, bounds, gbs, ham_diag=None):
    """the depth sweep on the members' own descriptors; params / moments rows padded with SENTINEL beyond each member"""
    return run_members(dev, 'depth', models, lrs, inputs, ys, bounds, gbs, ham_diag=ham_diag, sentinel=SENTINEL)


def _bitwise(dev, models, lrs, inputs, ys, bounds, gbs, ham_diag=None, variant='packed'):
    from quanonet_amd import _lib
    _lib.set_backward_variant(variant)
    try:
        got = _run_depth(dev, models, lrs, inputs, ys, bounds, gbs, ham_diag=ham_diag)
        for i, model in enumerate(models):
            P = _flat(model).numel()
            hd = None if ham_diag is None else torch.from_numpy(ham_diag[i]).to(dev)
            want = _run_single(dev, model.fused_desc(), model, inputs[i], ys[i], bounds, gbs, lrs[i], ham_diag=hd)
            for g, w, what in zip(got[:3], want[:3], ('params', 'exp_avg', 'exp_avg_sq')):
                assert torch.equal(g[i, :P], w), (i, what, float((g[i, :P] - w).abs().max()))
                assert bool((g[i, P:] == SENTINEL).all()), (i, what, 'row tail written')
            assert torch.equal(got[3][i, :, :P + 2], want[3]), (i, 'rows', float((got[3][i, :, :P + 2] - want[3]).abs().max()))
    finally:
        _lib.set_backward_variant('auto')


Q2_NETS = [(5, 2, 5, 2), (40, 2, 10, 2), (60, 2, 30, 2)]


def test_q2_depths_x_seeds_bitwise(dev):
    bounds, gbs = _schedule(100, 3)
    cells = [(net, s) for net in Q2_NETS for s in range(2)]
    inputs, ys = _data(len(cells), bounds[-1], (10, 1), 1100)
    models = [_quanonet(2, 10, 1, net, s, scale_coeff=0.1, if_trainable_freq=True) for net, s in cells]
    _bitwise(dev, models, [1e-3 * (1 + i) for i in range(len(cells))], inputs, ys, bounds, gbs)


@pytest.mark.parametrize('n, nets', [(3, [(4, 2, 2, 2), (1, 2, 9, 2), (12, 2, 6, 2)]), (6, [(2, 2, 1, 2), (1, 2, 4, 2)])])
def test_other_qubit_counts_bitwise(dev, n, nets):
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(len(nets), bounds[-1], (6, 2), 1200 + n)
    models = [_quanonet(n, 6, 2, net, i, scale_coeff=0.1, if_trainable_freq=True) for i, net in enumerate(nets)]
    _bitwise(dev, models, [1e-3] * len(nets), inputs, ys, bounds, gbs)


def test_fixed_frequency_short_last_batch_bitwise(dev):
    nets = [(3, 1, 7, 1), (20, 1, 2, 1), (9, 1, 9, 1)]
    bounds, gbs = _schedule(100, 3, last=37)
    inputs, ys = _data(3, bounds[-1], (10, 1), 1300)
    models = [_quanonet(2, 10, 1, net, i, scale_coeff=s, if_trainable_freq=False) for i, (net, s) in
              enumerate(zip(nets, (0.1, 0.01, 0.3)))]
    _bitwise(dev, models, [1e-3, 2e-3, 5e-4], inputs, ys, bounds, gbs)


def test_mixed_xz_readout_bitwise(dev):
    nets = [(5, 2, 5, 2), (30, 2, 10, 2), (8, 2, 40, 2)]
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(3, bounds[-1], (10, 1), 1400)
    models = [_quanonet(2, 10, 1, net, i, scale_coeff=0.1, if_trainable_freq=True, ham_pauli='XZX'[i],
                        ham_bound=(-1.0 - i, 2.0)) for i, net in enumerate(nets)]
    _bitwise(dev, models, [1e-3] * 3, inputs, ys, bounds, gbs)


def test_ham_diag_sweep_bitwise(dev):
    nets = [(10, 2, 10, 2), (50, 2, 20, 2), (4, 2, 60, 2)]
    spectra = ([-5, 5, 5, 5], [-5, 0, 0, 5], [-5, -2.5, 2.5, 5])
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(3, bounds[-1], (10, 1), 1500)
    models = [_quanonet(2, 10, 1, net, i, scale_coeff=0.1, if_trainable_freq=True, ham_diag=np.asarray(s, np.float64))
              for i, (net, s) in enumerate(zip(nets, spectra))]
    hd = [m.quantum_layer.ham_diag.detach().cpu().numpy().astype(np.float64) for m in models]
    _bitwise(dev, models, [1e-3] * 3, inputs, ys, bounds, gbs, ham_diag=hd)


def test_heaqnn_depth_grid_bitwise(dev):
    nets = [(2, 2), (7, 2), (4, 2)]
    bounds, gbs = _schedule(100, 3, last=51)
    inputs, ys = _data(3, bounds[-1], (4,), 1600)
    models = [_heaqnn(3, 4, net, i) for i, net in enumerate(nets)]
    _bitwise(dev, models, [1e-3] * 3, inputs, ys, bounds, gbs)


def test_members_match_the_oracle(dev):
    from oracle import hea_oracle as O
    from oracle import c_oracle as C
    nets = [(5, 2, 5, 2), (12, 2, 3, 2), (2, 2, 9, 2)]
    bounds, gbs = _schedule(100, 2, last=64)
    inputs, ys = _data(3, bounds[-1], (10, 1), 1700)
    models = [_quanonet(2, 10, 1, net, i, scale_coeff=0.1, if_trainable_freq=True) for i, net in enumerate(nets)]
    got_p, _, _, got_rows = _run_depth(dev, models, [1e-3] * 3, inputs, ys, bounds, gbs)
    for i, (model, net) in enumerate(zip(models, nets)):
        def lg(sd, ins, y, gb, net=net):
            loss, grads, _ = O.quanonet_loss_and_grads(sd, ins[0], ins[1], y, 2, net, ham_bound=(-5.0, 5.0), batch_total=gb,
                                                       engine=C)
            return loss, grads
        want_rows, want_p = _oracle_adam(model, lg, inputs[i], ys[i], bounds, gbs, 1e-3)
        P = want_p.size
        err_r = np.abs(got_rows[i][:, :P + 2].numpy() - want_rows).max() / max(1.0, np.abs(want_rows).max())
        err_p = np.abs(got_p[i][:P].numpy() - want_p).max() / max(1.0, np.abs(want_p).max())
        assert err_r < 1e-10 and err_p < 1e-10, (i, err_r, err_p)


def test_q10_grid_runs_each_member_alone(dev):
    nets = [(1, 1, 2, 1), (2, 1, 1, 1)]
    bounds, gbs = _schedule(64, 2)
    inputs, ys = _data(2, bounds[-1], (4, 2), 1800)
    models = [_quanonet(10, 4, 2, net, i, scale_coeff=0.1, if_trainable_freq=True) for i, net in enumerate(nets)]
    got = _run_depth(dev, models, [1e-3, 2e-3], inputs, ys, bounds, gbs)
    for i, model in enumerate(models):
        P = _flat(model).numel()
        want = _run_single(dev, model.fused_desc(), model, inputs[i], ys[i], bounds, gbs, [1e-3, 2e-3][i])
        for g, w in zip(got[:3], want[:3]):
            assert torch.equal(g[i, :P], w) and bool((g[i, P:] == SENTINEL).all())
        assert torch.equal(got[3][i, :, :P + 2], want[3])


BASE = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'scale_coeff': 0.001, 'if_trainable_freq': 'true',
        'learning_rate': 1e-3, 'batch_size': 100, 'num_epochs': 3}


@pytest.mark.parametrize('variant', ['auto', 'packed'])
def test_depth_sweep_solver_matches_ptsolver_runs(dev, tmp_path, variant):
    from quanonet_amd import _lib
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.solver import PTSolver, set_random_seed
    from tests.test_ensemble import _antideriv
    cfgs = [dict(BASE, seed=s, net_size=[hb, 2, ht, 2], run_id=f'hb{hb}_ht{ht}_s{s}')
            for (hb, ht) in ((5, 5), (40, 10), (10, 30), (60, 30)) for s in (0,)] + \
           [dict(BASE, seed=1, net_size=[5, 2, 5, 2], run_id='hb5_ht5_s1')]
    data = _antideriv(1050)
    quiet = lambda *a, **k: None
    _lib.set_backward_variant(variant)
    try:
        sw = DepthSweepSolver([dict(c, prefix=str(tmp_path / 'sweep')) for c in cfgs], data, device=dev, log=quiet)
        hists = sw.train()
        metrics = sw.evaluate(hists)
        for c, h, mt, m in zip(cfgs, hists, metrics, sw.members):
            set_random_seed(c['seed'])
            solo = PTSolver(dict(c, prefix=str(tmp_path / 'solo')), data, device=dev, log=quiet)
            hs = solo.train()
            ms = solo.evaluate(hs)
            p_sw, p_solo = m.trainer.pflat.cpu(), solo.trainer.pflat.cpu()
            if variant == 'packed':              # the same variant forced for both: bitwise
                assert torch.equal(p_sw, p_solo), c
                assert h['loss_train'] == hs['loss_train'], c
                assert mt['rel_l2'] == ms['rel_l2'], c
                assert_checkpoints_bitwise(m.out_dir, solo.out_dir, c)
            else:                                 # AUTO: the single run may take the ZYZ kernels
                assert float((p_sw - p_solo).abs().max()) < 1e-10, c
                assert np.allclose(h['loss_train'], hs['loss_train'], rtol=1e-10, atol=0), c
                assert np.isclose(mt['rel_l2'], ms['rel_l2'], rtol=1e-10, atol=0), c
            for f in ('best_model.pt', 'final.pt'):
                a = torch.load(os.path.join(m.out_dir, f))
                b = torch.load(os.path.join(solo.out_dir, f))
                assert a.keys() == b.keys()
                for k in a:
                    if variant == 'packed':
                        assert torch.equal(a[k], b[k]), (c, f, k)
                    else:
                        assert float((a[k] - b[k]).abs().max()) < 1e-10, (c, f, k)
    finally:
        _lib.set_backward_variant('auto')
