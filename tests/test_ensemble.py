"""
Model ensemble on the GPU (qhea_model_ensemble_train_steps, quanonet_amd.ensemble.EnsembleSolver): R models of one
descriptor, every step of all members as one launch per kernel (member = blockIdx.y).

* under a forced backward variant every member's parameters, Adam moments and [grads | sse | sum y^2] rows are BITWISE those
  of model_train_steps run on that member alone (the headline model, R = 1, 3, 5, a shorter last step);
* under AUTO (the variant chosen for R x B rows: R = 8 leaves the quad-chain kernel) every member matches the oracle
  gradients + torch.optim.Adam at 1e-9;
* other shapes -- Q2 with the two-blocks-per-reduce-block record pairing, a Q3 net whose linear depths differ (a prep launch
  every step), a ham_diag read-out, X read-out, HEAQNN Q5, and HEAQNN Q8 (the R-sequential fallback) -- match the oracle;
* EnsembleSolver with seeds 0, 1, 2 matches three PTSolver runs made after set_random_seed(seed).
"""
import os

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from oracle import c_oracle as C
from tests.helpers import flat as _flat, heaqnn as _heaqnn, member_data as _data, oracle_adam as _oracle_adam
from tests.helpers import assert_checkpoints_bitwise, quanonet as _quanonet, run_members, run_single as _run_single, schedule as _schedule

pytestmark = pytest.mark.gpu
TOL = 1e-9
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _run_ensemble(dev, desc, models, inputs, ys, bounds, gbs, lr, ham_diag=None):
    return run_members(dev, 'ensemble', models, [lr] * len(models), inputs, ys, bounds, gbs, ham_diag=ham_diag, desc=desc)


HEADLINE = (5, 100, 2, (40, 2, 20, 2))


@pytest.mark.parametrize('variant', ['zquad', 'ztri', 'ztri2', 'zpacked'])
@pytest.mark.parametrize('R', [1, 3, 5])
def test_ensemble_is_bitwise_the_single_model_calls(dev, variant, R):
    from quanonet_amd import _lib
    n, b_in, t_in, net = HEADLINE
    bounds, gbs = _schedule(100, 3, last=37)
    inputs, ys = _data(R, bounds[-1], (b_in, t_in), 100 + R)
    models = [_quanonet(n, b_in, t_in, net, seed, scale_coeff=0.1, if_trainable_freq=True) for seed in range(R)]
    desc = models[0].fused_desc()
    _lib.set_backward_variant(variant)
    try:
        got = _run_ensemble(dev, desc, models, inputs, ys, bounds, gbs, 1e-3)
        for m in range(R):
            want = _run_single(dev, desc, models[m], inputs[m], ys[m], bounds, gbs, 1e-3)
            for g, w, what in zip(got, want, ('params', 'exp_avg', 'exp_avg_sq', 'rows')):
                assert torch.equal(g[m], w), (variant, R, m, what, float((g[m] - w).abs().max()))
    finally:
        _lib.set_backward_variant('auto')


def _check_against_oracle(dev, desc, models, inputs, ys, bounds, gbs, lossgrad, ham_diag=None, lr=1e-3):
    got_p, _, _, got_rows = _run_ensemble(dev, desc, models, inputs, ys, bounds, gbs, lr, ham_diag=ham_diag)
    for m, model in enumerate(models):
        want_rows, want_p = _oracle_adam(model, lossgrad, inputs[m], ys[m], bounds, gbs, lr)
        P = want_p.size
        err_r = np.abs(got_rows[m][:, :P + 2].numpy() - want_rows).max() / max(1.0, np.abs(want_rows).max())
        err_p = np.abs(got_p[m].numpy() - want_p).max()
        assert err_r < TOL and err_p < TOL, (m, err_r, err_p)


def _qlossgrad(n, net, ham_diag=None, ham_pauli='Z', scale=None):
    def f(sd, ins, y, gb):
        kw = {} if ham_diag is None else {'ham_diag': ham_diag}
        if scale is not None:
            kw['scale_coeff'] = scale
        if ham_pauli != 'Z':
            kw['ham_pauli'] = ham_pauli
        loss, grads, _ = O.quanonet_loss_and_grads(sd, ins[0], ins[1], y, n, net, batch_total=gb, engine=C, **kw)
        return loss, grads
    return f


def _hlossgrad(n, net):
    def f(sd, ins, y, gb):
        loss, grads, _ = O.heaqnn_loss_and_grads(sd, ins[0], y, n, net, batch_total=gb, engine=C)
        return loss, grads
    return f


@pytest.mark.parametrize('R', [5, 8])
def test_ensemble_auto_matches_the_oracle(dev, R):
    n, b_in, t_in, net = HEADLINE
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(R, bounds[-1], (b_in, t_in), 200 + R)
    models = [_quanonet(n, b_in, t_in, net, seed, scale_coeff=0.1, if_trainable_freq=True) for seed in range(R)]
    _check_against_oracle(dev, models[0].fused_desc(), models, inputs, ys, bounds, gbs, _qlossgrad(n, net))


def test_ensemble_q2_scale_repeat_and_fused_pairing(dev):
    for tf in (True, False):
        n, net = 2, (5, 1, 5, 1)
        bounds, gbs = _schedule(100, 3, last=61)
        inputs, ys = _data(3, bounds[-1], (10, 1), 300 + tf)
        models = [_quanonet(n, 10, 1, net, s, scale_coeff=0.3, if_trainable_freq=tf) for s in range(3)]
        _check_against_oracle(dev, models[0].fused_desc(), models, inputs, ys, bounds, gbs, _qlossgrad(n, net, scale=0.3))


def test_ensemble_q3_unequal_depths_prep_every_step(dev):
    n, net = 3, (2, 1, 2, 2)
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(3, bounds[-1], (7, 2), 400)
    models = [_quanonet(n, 7, 2, net, s, scale_coeff=0.2, if_trainable_freq=True) for s in range(3)]
    _check_against_oracle(dev, models[0].fused_desc(), models, inputs, ys, bounds, gbs, _qlossgrad(n, net))


def test_ensemble_ham_diag_readout(dev):
    n, net = 4, (2, 2, 2, 2)
    diag = np.random.default_rng(5).normal(size=1 << n)
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(3, bounds[-1], (6, 2), 500)
    models = [_quanonet(n, 6, 2, net, s, scale_coeff=0.2, if_trainable_freq=True, ham_diag=diag) for s in range(3)]
    hd = models[0].quantum_layer.ham_diag.to(dev)
    _check_against_oracle(dev, models[0].fused_desc(), models, inputs, ys, bounds, gbs, _qlossgrad(n, net, ham_diag=diag),
                          ham_diag=hd)


def test_ensemble_x_readout(dev):
    n, net = 3, (2, 2, 2, 2)
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(3, bounds[-1], (6, 2), 600)
    models = [_quanonet(n, 6, 2, net, s, scale_coeff=0.2, if_trainable_freq=True, ham_pauli='X') for s in range(3)]
    _check_against_oracle(dev, models[0].fused_desc(), models, inputs, ys, bounds, gbs, _qlossgrad(n, net, ham_pauli='X'))


@pytest.mark.parametrize('n', [5, 8])
def test_ensemble_heaqnn(dev, n):
    net = (3, 2)
    bounds, gbs = _schedule(100, 3, last=50)
    inputs, ys = _data(3, bounds[-1], (4,), 700 + n)
    models = [_heaqnn(n, 4, net, s) for s in range(3)]
    _check_against_oracle(dev, models[0].fused_desc(), models, inputs, ys, bounds, gbs, _hlossgrad(n, net))


def _antideriv(rows):
    tr = np.load(os.path.join(HERE, 'golden', 'antideriv_train.npz'), allow_pickle=False)
    te = np.load(os.path.join(HERE, 'golden', 'antideriv_demo.npz'), allow_pickle=False)
    ns = tr['x'].shape[1]
    return {'train_branch_input': np.repeat(tr['u0'], ns, axis=0)[:rows], 'train_trunk_input': tr['x'].reshape(-1, 1)[:rows],
            'train_output': tr['u'].reshape(-1, 1)[:rows],
            'test_branch_input': np.repeat(te['u0'], te['u'].shape[1], axis=0)[:500],
            'test_trunk_input': np.tile(te['x'], te['u'].shape[0]).reshape(-1, 1)[:500],
            'test_output': te['u'].reshape(-1, 1)[:500]}


@pytest.mark.parametrize('variant', ['auto', 'ztri'])
def test_ensemble_solver_matches_ptsolver_runs(dev, tmp_path, variant):
    from quanonet_amd import _lib
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.solver import PTSolver, set_random_seed
    data = _antideriv(1050)
    base = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'net_size': [5, 1, 5, 1],
            'scale_coeff': 0.001, 'if_trainable_freq': 'true', 'learning_rate': 1e-3, 'batch_size': 100, 'num_epochs': 2}
    seeds = (0, 1, 2)
    quiet = lambda *a, **k: None
    _lib.set_backward_variant(variant)
    try:
        ens = EnsembleSolver([dict(base, seed=s, run_id=f'seed{s}', prefix=str(tmp_path / 'ens')) for s in seeds], data,
                             device=dev, log=quiet)
        hists = ens.train()
        for s, h, m in zip(seeds, hists, ens.members):
            set_random_seed(s)
            solo = PTSolver(dict(base, seed=s, run_id=f'seed{s}', prefix=str(tmp_path / 'solo')), data, device=dev, log=quiet)
            hs = solo.train()
            p_ens, p_solo = m.trainer.pflat.cpu(), solo.trainer.pflat.cpu()
            if variant == 'auto':
                assert float((p_ens - p_solo).abs().max()) < TOL, s
                assert np.allclose(h['loss_train'], hs['loss_train'], rtol=TOL, atol=0), s
            else:                                    # the same variant forced for both: bitwise
                assert torch.equal(p_ens, p_solo), s
                assert h['loss_train'] == hs['loss_train'], s
                assert_checkpoints_bitwise(m.out_dir, solo.out_dir, s)
            for f in ('best_model.pt', 'final.pt', 'final.npz'):
                assert os.path.exists(os.path.join(m.out_dir, f)), (s, f)
        metrics = ens.evaluate(hists)
        assert len(metrics) == 3 and all(np.isfinite(mt['rel_l2']) for mt in metrics)
    finally:
        _lib.set_backward_variant('auto')
