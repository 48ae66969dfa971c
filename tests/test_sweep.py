"""
Model sweep on the GPU (qhea_model_sweep_train_steps, quanonet_amd.sweep.SweepSolver): R models of one circuit shape whose
read-out, fixed scale and learning rate differ per member, every step of all members as one launch per kernel.

* under a forced backward variant every member's parameters, Adam moments and [grads | sse | sum y^2] rows are BITWISE those
  of model_train_steps on that member alone with its own descriptor and learning rate (headline model, R = 1, 5, 12);
* fixed-frequency scales, and a mixed X / Y / Z read-out (kernels of an X / Y model for the whole launch), bitwise likewise;
* under AUTO: mixed Pauli, per-member ham_diag spectra, the HEAQNN Q8 fallback and R = 50 at Exp. 2's shape match the oracle
  gradients + torch.optim.Adam at 1e-9; a uniform table is bitwise the ensemble call;
* SweepSolver matches the PTSolver runs its configs describe, checkpoints included.
"""
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_checkpoints_bitwise, run_members
from tests.test_ensemble import _antideriv, _data, _flat, _oracle_adam, _quanonet, _run_ensemble, _run_single, _schedule

pytestmark = pytest.mark.gpu
TOL = 1e-9
HEADLINE = (5, 100, 2, (40, 2, 20, 2))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _run_sweep(dev, desc, models, descs, lrs, inputs, ys, bounds, gbs, ham_diag=None):
    """the sweep on `desc`'s shape; member m reads out as descs[m] (the members' own descriptors) with lrs[m]"""
    assert all(d.ham_pauli == m.fused_desc().ham_pauli and d.scale_coeff == m.fused_desc().scale_coeff
               for d, m in zip(descs, models))
    return run_members(dev, 'sweep', models, lrs, inputs, ys, bounds, gbs, ham_diag=ham_diag, desc=desc)


def _two_pipes(dev, variant, R, B):
    """ZTRI2 puts two sample groups in one workgroup (their gradient sums added in LDS) once the launch has more sample groups
    than the device has CUs: R x B rows can reach that where B rows alone cannot, and no single-model call then runs the
    kernel configuration the sweep chose (n = 5: two samples per group)"""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return variant == 'ztri2' and R * ((B + 1) // 2) > cus >= (B + 1) // 2


def _bitwise(dev, variant, models, lrs, inputs, ys, bounds, gbs):
    from quanonet_amd import _lib
    descs = [m.fused_desc() for m in models]
    exact = not any(_two_pipes(dev, variant, len(models), b) for b in gbs)
    _lib.set_backward_variant(variant)
    try:
        got = _run_sweep(dev, descs[0], models, descs, lrs, inputs, ys, bounds, gbs)
        for m in range(len(models)):
            want = _run_single(dev, descs[m], models[m], inputs[m], ys[m], bounds, gbs, lrs[m])
            for g, w, what in zip(got, want, ('params', 'exp_avg', 'exp_avg_sq', 'rows')):
                if exact:
                    assert torch.equal(g[m], w), (variant, m, what, float((g[m] - w).abs().max()))
                else:                   # the same arithmetic in another summation order
                    err = float((g[m] - w).abs().max()) / max(1.0, float(w.abs().max()))
                    assert err < 1e-12, (variant, m, what, err)
    finally:
        _lib.set_backward_variant('auto')


def _bounds(m):
    return (-1.0 - m, 1.0 + 0.5 * m)


@pytest.mark.parametrize('variant', ['zquad', 'ztri', 'ztri2', 'zpacked'])
@pytest.mark.parametrize('R', [1, 5, 12])
def test_sweep_is_bitwise_the_single_model_calls(dev, variant, R):
    n, b_in, t_in, net = HEADLINE
    bounds, gbs = _schedule(100, 3, last=37)
    inputs, ys = _data(R, bounds[-1], (b_in, t_in), 900 + R)
    models = [_quanonet(n, b_in, t_in, net, m, scale_coeff=0.1, if_trainable_freq=True, ham_bound=_bounds(m)) for m in range(R)]
    _bitwise(dev, variant, models, [1e-3 * (1 + m) for m in range(R)], inputs, ys, bounds, gbs)


@pytest.mark.parametrize('variant', ['ztri', 'zquad'])
def test_sweep_fixed_frequency_scales_bitwise(dev, variant):
    n, b_in, t_in, net = HEADLINE
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(3, bounds[-1], (b_in, t_in), 950)
    models = [_quanonet(n, b_in, t_in, net, m, scale_coeff=s, if_trainable_freq=False) for m, s in enumerate((0.1, 0.01, 0.001))]
    _bitwise(dev, variant, models, [1e-3] * 3, inputs, ys, bounds, gbs)


def _mixed(R=3):
    n, b_in, t_in, net = HEADLINE
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(R, bounds[-1], (b_in, t_in), 960)
    models = [_quanonet(n, b_in, t_in, net, m, scale_coeff=0.1, if_trainable_freq=True, ham_pauli='XYZ'[m % 3],
                        ham_bound=_bounds(m)) for m in range(R)]
    return models, inputs, ys, bounds, gbs


@pytest.mark.parametrize('variant', ['ztri', 'ztri2', 'zpacked'])
def test_sweep_mixed_pauli_bitwise(dev, variant):
    models, inputs, ys, bounds, gbs = _mixed()
    _bitwise(dev, variant, models, [1e-3, 2e-3, 3e-3], inputs, ys, bounds, gbs)


def _against_oracle(dev, models, lrs, inputs, ys, bounds, gbs, lossgrads, ham_diag=None):
    descs = [m.fused_desc() for m in models]
    got_p, _, _, got_rows = _run_sweep(dev, descs[0], models, descs, lrs, inputs, ys, bounds, gbs, ham_diag=ham_diag)
    for m, model in enumerate(models):
        want_rows, want_p = _oracle_adam(model, lossgrads[m], inputs[m], ys[m], bounds, gbs, lrs[m])
        P = want_p.size
        err_r = np.abs(got_rows[m][:, :P + 2].numpy() - want_rows).max() / max(1.0, np.abs(want_rows).max())
        err_p = np.abs(got_p[m].numpy() - want_p).max()
        assert err_r < TOL and err_p < TOL, (m, err_r, err_p)


def _qlg(n, net, ham_bound=(-5.0, 5.0), ham_pauli='Z', ham_diag=None):
    """oracle loss / gradients of one QuanONet member"""
    from oracle import hea_oracle as O
    from oracle import c_oracle as C

    def f(sd, ins, y, gb):
        loss, grads, _ = O.quanonet_loss_and_grads(sd, ins[0], ins[1], y, n, net, ham_bound=ham_bound, batch_total=gb,
                                                   ham_pauli=ham_pauli, ham_diag=ham_diag, engine=C)
        return loss, grads
    return f


def test_sweep_mixed_pauli_auto_matches_the_oracle(dev):
    models, inputs, ys, bounds, gbs = _mixed()
    n, _, _, net = HEADLINE
    lg = [_qlg(n, net, ham_bound=_bounds(m), ham_pauli='XYZ'[m]) for m in range(3)]
    _against_oracle(dev, models, [1e-3, 2e-3, 3e-3], inputs, ys, bounds, gbs, lg)


SPECTRA = ([-5, 5, 5, 5], [-5, -5, -5, 5], [-5, 0, 0, 5], [-5, -2.5, 2.5, 5])


def test_sweep_ham_diag_spectra_match_the_oracle(dev):
    n, net = 2, (50, 2, 50, 2)
    bounds, gbs = _schedule(100, 3)
    inputs, ys = _data(4, bounds[-1], (10, 1), 970)
    diags = [np.asarray(s, dtype=np.float64) for s in SPECTRA]
    models = [_quanonet(n, 10, 1, net, m, scale_coeff=0.1, if_trainable_freq=True, ham_diag=d) for m, d in enumerate(diags)]
    hd = [m.quantum_layer.ham_diag.detach().cpu().numpy() for m in models]
    _against_oracle(dev, models, [1e-3] * 4, inputs, ys, bounds, gbs, [_qlg(n, net, ham_diag=d) for d in diags],
                    ham_diag=hd)


def test_sweep_heaqnn_q8_fallback_matches_the_oracle(dev):
    from oracle import c_oracle as C
    from oracle import hea_oracle as O
    from quanonet_amd.models import HEAQNNPT
    n, net = 8, (3, 2)
    bounds, gbs = _schedule(100, 3, last=50)
    inputs, ys = _data(3, bounds[-1], (4,), 980)
    cells = [('Z', (-5, 5), 0.1, 1e-3), ('X', (-2, 1), 0.01, 2e-3), ('Y', (-1, 3), 0.3, 5e-4)]
    models = []
    for m, (p, hb, sc, _) in enumerate(cells):
        torch.manual_seed(m)
        models.append(HEAQNNPT(n, 4, net, scale_coeff=sc, if_trainable_freq=False, ham_bound=hb, ham_pauli=p).double())

    def lossgrad(p, hb, sc):
        def f(sd, ins, y, gb):
            loss, grads, _ = O.heaqnn_loss_and_grads(sd, ins[0], y, n, net, ham_bound=hb, batch_total=gb, ham_pauli=p,
                                                     scale_coeff=sc, engine=C)
            return loss, grads
        return f
    _against_oracle(dev, models, [c[3] for c in cells], inputs, ys, bounds, gbs, [lossgrad(p, hb, sc) for p, hb, sc, _ in cells])


def test_sweep_uniform_table_is_bitwise_the_ensemble(dev):
    n, b_in, t_in, net = HEADLINE
    bounds, gbs = _schedule(100, 3, last=37)
    inputs, ys = _data(5, bounds[-1], (b_in, t_in), 990)
    models = [_quanonet(n, b_in, t_in, net, m, scale_coeff=0.1, if_trainable_freq=True) for m in range(5)]
    d = models[0].fused_desc()
    got = _run_sweep(dev, d, models, [d] * 5, [1e-3] * 5, inputs, ys, bounds, gbs)
    want = _run_ensemble(dev, d, models, inputs, ys, bounds, gbs, 1e-3)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_sweep_r50_exp2_shape_matches_the_oracle(dev):
    n, b_in, t_in, net = 5, 100, 2, (20, 2, 10, 2)
    R = 50
    bounds, gbs = _schedule(100, 2)
    inputs, ys = _data(R, bounds[-1], (b_in, t_in), 999)
    hbs = [(-b, b) for b in range(1, 11)]
    models = [_quanonet(n, b_in, t_in, net, m % 5, scale_coeff=0.01, if_trainable_freq=True, ham_bound=hbs[m // 5])
              for m in range(R)]
    lg = [_qlg(n, net, ham_bound=hbs[m // 5]) for m in range(R)]
    _against_oracle(dev, models, [1e-3] * R, inputs, ys, bounds, gbs, lg)


BASE = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'net_size': [5, 1, 5, 1], 'scale_coeff': 0.001,
        'if_trainable_freq': 'true', 'learning_rate': 1e-3, 'batch_size': 100, 'num_epochs': 3}


def _other_operator(rows):
    d = _antideriv(rows)
    rng = np.random.default_rng(7)
    return dict(d, train_output=np.sin(3 * d['train_trunk_input']) * d['train_branch_input'][:, :1] + 0.1 * rng.normal(
        size=d['train_output'].shape))


def _cells():
    a = _antideriv(1050)
    return {
        'bounds_x_seeds': ([dict(BASE, seed=s, ham_bound=[-b, b], run_id=f'b{b}_s{s}') for b in (2, 5) for s in (0, 1)], a),
        'operators': ([dict(BASE, seed=0, operator=op, run_id='s0') for op in ('Antideriv', 'Other')],
                      [a, _other_operator(1050)]),
        'fixed_scales': ([dict(BASE, seed=0, if_trainable_freq='false', scale_coeff=sc, run_id=f'sc{sc}')
                          for sc in (0.1, 0.01, 0.001)], a),
        'lr_steplr': ([dict(BASE, seed=1, learning_rate=lr, lr_scheduler='step', lr_scheduler_kwargs={'step_size': 1, 'gamma': 0.5},
                            run_id=f'lr{lr}') for lr in (1e-3, 5e-3)], a),
    }


@pytest.mark.parametrize('variant', ['auto', 'ztri'])
@pytest.mark.parametrize('cell', ['bounds_x_seeds', 'operators', 'fixed_scales', 'lr_steplr'])
def test_sweep_solver_matches_ptsolver_runs(dev, tmp_path, variant, cell):
    from quanonet_amd import _lib
    from quanonet_amd.solver import PTSolver, set_random_seed
    from quanonet_amd.sweep import SweepSolver
    cfgs, data = _cells()[cell]
    datas = data if isinstance(data, list) else [data] * len(cfgs)
    quiet = lambda *a, **k: None
    _lib.set_backward_variant(variant)
    try:
        sw = SweepSolver([dict(c, prefix=str(tmp_path / 'sweep')) for c in cfgs], data, device=dev, log=quiet)
        hists = sw.train()
        dirs = set()
        for c, d, h, m in zip(cfgs, datas, hists, sw.members):
            set_random_seed(c['seed'])
            solo = PTSolver(dict(c, prefix=str(tmp_path / 'solo')), d, device=dev, log=quiet)
            hs = solo.train()
            p_sw, p_solo = m.trainer.pflat.cpu(), solo.trainer.pflat.cpu()
            if variant == 'auto':
                assert float((p_sw - p_solo).abs().max()) < TOL, c
                assert np.allclose(h['loss_train'], hs['loss_train'], rtol=TOL, atol=0), c
            else:                                    # the same variant forced for both: bitwise
                assert torch.equal(p_sw, p_solo), c
                assert h['loss_train'] == hs['loss_train'], c
                assert_checkpoints_bitwise(m.out_dir, solo.out_dir, c)
            assert m.trainer.optimizer.param_groups[0]['lr'] == solo.trainer.optimizer.param_groups[0]['lr'], c
            assert m.out_dir.startswith(str(tmp_path / 'sweep')) and m.out_dir not in dirs
            dirs.add(m.out_dir)
            for f in ('best_model.pt', 'final.pt', 'final.npz'):
                assert os.path.exists(os.path.join(m.out_dir, f)), (c, f)
        metrics = sw.evaluate(hists)
        assert len(metrics) == len(cfgs) and all(np.isfinite(mt['rel_l2']) for mt in metrics)
    finally:
        _lib.set_backward_variant('auto')
