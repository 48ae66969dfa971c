"""
Qubit sweep on the GPU (qhea_model_qubit_sweep_train_steps, quanonet_amd.qubit_sweep.QubitSweepSolver): R models whose qubit
counts and circuit depths differ (and read-out, scale, learning rate); every step of the n <= 9 members is one prep launch, one
backward launch per register class and one reduce launch.

* every member's parameters, Adam moments and [grads | sse | sum y^2] rows are BITWISE those of model_train_steps on that member
  alone under the packed backward variant -- a grid over every register class, fixed frequency with a short last batch, mixed
  X / Z read-out, per-member ham_diag spectra of 2^n_m entries, HEAQNN, an n = 10 member among wave-resident ones; the rows'
  tails beyond each member's vector stay untouched;
* a grid of one qubit count gives what the depth sweep gives; members match the CPU oracle + torch.optim.Adam at 1e-10;
* QubitSweepSolver matches the PTSolver runs its configs describe, checkpoints and evaluate metrics included.
"""
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_checkpoints_bitwise, run_members
from tests.test_depth_sweep import _run_depth
from tests.test_ensemble import _data, _flat, _heaqnn, _oracle_adam, _quanonet, _run_single, _schedule

pytestmark = pytest.mark.gpu
SENTINEL = 12345.678


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _run_qubit(dev, models, lrs, inputs, ys, bounds, gbs, ham_diag=None):
    """the qubit sweep on the members' own descriptors; params / moments rows padded with SENTINEL beyond each member"""
    return run_members(dev, 'qubit', models, lrs, inputs, ys, bounds, gbs, ham_diag=ham_diag, sentinel=SENTINEL,
                       rows_sentinel=SENTINEL)


def _bitwise(dev, models, lrs, inputs, ys, bounds, gbs, ham_diag=None):
    from quanonet_amd import _lib
    _lib.set_backward_variant('packed')
    try:
        got = _run_qubit(dev, models, lrs, inputs, ys, bounds, gbs, ham_diag=ham_diag)
        for i, model in enumerate(models):
            P = _flat(model).numel()
            hd = None if ham_diag is None else torch.from_numpy(np.asarray(ham_diag[i], np.float64)).to(dev)
            want = _run_single(dev, model.fused_desc(), model, inputs[i], ys[i], bounds, gbs, lrs[i], ham_diag=hd)
            for g, w, what in zip(got[:3], want[:3], ('params', 'exp_avg', 'exp_avg_sq')):
                assert torch.equal(g[i, :P], w), (i, what, float((g[i, :P] - w).abs().max()))
                assert bool((g[i, P:] == SENTINEL).all()), (i, what, 'row tail written')
            assert torch.equal(got[3][i, :, :P + 2], want[3]), (i, 'rows', float((got[3][i, :, :P + 2] - want[3]).abs().max()))
            assert bool((got[3][i, :, P + 2:] == SENTINEL).all()), (i, 'gradient row tail written')
    finally:
        _lib.set_backward_variant('auto')


def test_every_register_class_bitwise(dev):
    # n = 2 | 3, 5, 6 | 8, 9: every class, two depth pairs, two seeds
    bounds, gbs = _schedule(100, 3)
    cells = [(n, net, s) for n in (2, 3, 5, 6, 8, 9) for net in ((2, 2, 3, 2), (4, 2, 1, 2)) for s in range(2)]
    inputs, ys = _data(len(cells), bounds[-1], (10, 1), 2100)
    models = [_quanonet(n, 10, 1, net, 7 * n + s, scale_coeff=0.1, if_trainable_freq=True) for n, net, s in cells]
    _bitwise(dev, models, [1e-3 * (1 + i % 5) for i in range(len(cells))], inputs, ys, bounds, gbs)


def test_fixed_frequency_short_last_batch_bitwise(dev):
    cells = [(2, (3, 1, 7, 1), 0.1), (4, (5, 1, 2, 1), 0.01), (7, (2, 1, 2, 1), 0.3), (8, (1, 1, 2, 1), 0.2)]
    bounds, gbs = _schedule(100, 3, last=37)
    inputs, ys = _data(len(cells), bounds[-1], (10, 1), 2200)
    models = [_quanonet(n, 10, 1, net, i, scale_coeff=s, if_trainable_freq=False) for i, (n, net, s) in enumerate(cells)]
    _bitwise(dev, models, [1e-3, 2e-3, 5e-4, 1e-3], inputs, ys, bounds, gbs)


def test_mixed_xz_readout_bitwise(dev):
    cells = [(2, (5, 2, 5, 2)), (5, (3, 2, 1, 2)), (9, (1, 2, 2, 2))]
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(3, bounds[-1], (10, 1), 2300)
    models = [_quanonet(n, 10, 1, net, i, scale_coeff=0.1, if_trainable_freq=True, ham_pauli='XZX'[i],
                        ham_bound=(-1.0 - i, 2.0)) for i, (n, net) in enumerate(cells)]
    _bitwise(dev, models, [1e-3] * 3, inputs, ys, bounds, gbs)


def test_ham_diag_per_member_bitwise(dev):
    cells = [(2, (10, 2, 10, 2)), (3, (4, 2, 2, 2)), (6, (2, 2, 3, 2))]
    rng = np.random.default_rng(2400)
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(3, bounds[-1], (10, 1), 2400)
    models = [_quanonet(n, 10, 1, net, i, scale_coeff=0.1, if_trainable_freq=True,
                        ham_diag=np.sort(rng.uniform(-5, 5, size=1 << n)))
              for i, (n, net) in enumerate(cells)]
    hd = [m.quantum_layer.ham_diag.detach().cpu().numpy().astype(np.float64) for m in models]
    assert [len(h) for h in hd] == [4, 8, 64]
    _bitwise(dev, models, [1e-3] * 3, inputs, ys, bounds, gbs, ham_diag=hd)


def test_heaqnn_qubit_grid_bitwise(dev):
    cells = [(2, (2, 2)), (4, (7, 2)), (7, (3, 2)), (9, (2, 2))]
    bounds, gbs = _schedule(100, 3, last=51)
    inputs, ys = _data(len(cells), bounds[-1], (4,), 2500)
    models = [_heaqnn(n, 4, net, i) for i, (n, net) in enumerate(cells)]
    _bitwise(dev, models, [1e-3] * len(cells), inputs, ys, bounds, gbs)


def test_n10_member_among_wave_resident_ones_bitwise(dev):
    cells = [(10, (1, 1, 2, 1)), (3, (2, 1, 1, 1)), (8, (1, 1, 1, 1))]
    bounds, gbs = _schedule(64, 2)
    inputs, ys = _data(len(cells), bounds[-1], (4, 2), 2600)
    models = [_quanonet(n, 4, 2, net, i, scale_coeff=0.1, if_trainable_freq=True) for i, (n, net) in enumerate(cells)]
    _bitwise(dev, models, [1e-3, 2e-3, 5e-4], inputs, ys, bounds, gbs)


def test_one_qubit_count_matches_the_depth_sweep(dev):
    from quanonet_amd import _lib
    nets = [(5, 2, 5, 2), (12, 2, 3, 2), (2, 2, 9, 2)]
    bounds, gbs = _schedule(100, 3, last=40)
    inputs, ys = _data(3, bounds[-1], (10, 1), 2700)
    models = [_quanonet(5, 10, 1, net, i, scale_coeff=0.1, if_trainable_freq=True) for i, net in enumerate(nets)]
    _lib.set_backward_variant('packed')
    try:
        a = _run_qubit(dev, models, [1e-3, 2e-3, 3e-3], inputs, ys, bounds, gbs)
        b = _run_depth(dev, models, [1e-3, 2e-3, 3e-3], inputs, ys, bounds, gbs)
    finally:
        _lib.set_backward_variant('auto')
    for x, z in zip(a[:3], b[:3]):
        assert torch.equal(x, z)
    for i, m in enumerate(models):
        P = _flat(m).numel()
        assert torch.equal(a[3][i, :, :P + 2], b[3][i, :, :P + 2]), i


def test_members_match_the_oracle(dev):
    from oracle import hea_oracle as O
    from oracle import c_oracle as C
    cells = [(2, (5, 2, 5, 2)), (4, (3, 2, 2, 2)), (7, (1, 2, 2, 2))]
    bounds, gbs = _schedule(100, 2, last=64)
    inputs, ys = _data(3, bounds[-1], (10, 1), 2800)
    models = [_quanonet(n, 10, 1, net, i, scale_coeff=0.1, if_trainable_freq=True) for i, (n, net) in enumerate(cells)]
    got_p, _, _, got_rows = _run_qubit(dev, models, [1e-3] * 3, inputs, ys, bounds, gbs)
    for i, (model, (n, net)) in enumerate(zip(models, cells)):
        def lg(sd, ins, y, gb, net=net, n=n):
            loss, grads, _ = O.quanonet_loss_and_grads(sd, ins[0], ins[1], y, n, net, ham_bound=(-5.0, 5.0), batch_total=gb,
                                                       engine=C)
            return loss, grads
        want_rows, want_p = _oracle_adam(model, lg, inputs[i], ys[i], bounds, gbs, 1e-3)
        P = want_p.size
        err_r = np.abs(got_rows[i][:, :P + 2].numpy() - want_rows).max() / max(1.0, np.abs(want_rows).max())
        err_p = np.abs(got_p[i][:P].numpy() - want_p).max() / max(1.0, np.abs(want_p).max())
        assert err_r < 1e-10 and err_p < 1e-10, (i, err_r, err_p)


BASE = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'scale_coeff': 0.001, 'if_trainable_freq': 'true',
        'learning_rate': 1e-3, 'batch_size': 100, 'num_epochs': 3}


@pytest.mark.parametrize('variant', ['auto', 'packed'])
def test_qubit_sweep_solver_matches_ptsolver_runs(dev, tmp_path, variant):
    from quanonet_amd import _lib
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    from quanonet_amd.solver import PTSolver, set_random_seed
    from tests.test_ensemble import _antideriv
    cfgs = [dict(BASE, seed=s, num_qubits=n, net_size=[hb, 2, ht, 2], run_id=f'q{n}_hb{hb}_ht{ht}_s{s}')
            for (n, hb, ht, s) in ((2, 5, 5, 0), (2, 10, 5, 1), (4, 3, 2, 0), (6, 2, 2, 0), (8, 1, 2, 0))]
    data = _antideriv(1050)
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
            if variant == 'packed':              # the same variant forced for both: bitwise
                assert torch.equal(p_sw, p_solo), c
                assert h['loss_train'] == hs['loss_train'], c
                assert mt['rel_l2'] == ms['rel_l2'], c
                assert_checkpoints_bitwise(m.out_dir, solo.out_dir, c)
            else:                                 # AUTO: the single run may take other backward kernels
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
