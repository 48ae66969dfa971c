"""
Noise-aware training on the GPU (qhea_model_loss_grad_noisy_exact / qhea_model_train_steps_noisy_exact, quanonet_amd.noise,
DataParallelTrainer / PTSolver with train_noise) against the numpy helper tests/density_grad_reference.py: the whole [P + 2]
buffer and pred for every shape, noiseless = the ideal call, pred = the exact noisy forward, determinism, shards, batch
independence, train_steps = the loop of single calls, Adam against torch, errors, graph capture, the solvers.
Tolerance against the helper: atol 1e-10, the one the HIP path is held to against the oracle.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import density_grad_reference as DG
from tests import helpers as H
from tests.test_noisy_forward import _inputs, _model, _solver_data

pytestmark = pytest.mark.gpu
ATOL = 1e-10
P3 = (0.03, 0.08, 0.04)
READOUTS = ('Z', 'X', 'Y', 'diag')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _noise(p=P3):
    from quanonet_amd.noise import NoiseModel
    return NoiseModel(p1=p[0], p2=p[1], readout=p[2])


def _targets(rows, dev, seed=0):
    return torch.tensor(np.random.default_rng(seed + 100).normal(scale=0.7, size=rows), device=dev)


def _diag(m):
    q = m.quantum_layer
    return q.ham_diag if q.use_full_ham else None


def _call(m, ins, y, p=P3, inv=None, want_pred=True, flat=None):
    """(grad[P+2], pred[B]) of one qhea_model_loss_grad_noisy_exact call as numpy arrays"""
    from quanonet_amd import _lib
    flat = H.flat(m) if flat is None else flat
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device) if want_pred else None
    _lib.model_loss_grad_noisy_exact(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat, _noise(p).params(),
                                     1.0 / rows if inv is None else inv, grad, ham_diag=_diag(m), pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (pred.cpu().numpy() if want_pred else None)


def _helper(m, ins, y, p=P3, inv=None, flat=None):
    flat = H.flat(m) if flat is None else flat
    rows = ins[0].shape[0]
    return DG.model_loss_grad(DG.spec_of(m), flat.cpu().numpy(), ins[0].cpu().numpy(),
                              ins[1].cpu().numpy() if len(ins) > 1 else None, y.cpu().numpy(), *p,
                              1.0 / rows if inv is None else inv)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_against_the_helper(dev, n, kind):
    for trainable in (True, False):
        for readout in READOUTS:
            m = _model(kind, n, trainable, readout, seed=n).to(dev)
            assert DG.log10_amplification(n, [(n, 1)] * 4, P3[0], P3[1]) < 2.0          # far inside the guard
            for rows in (1, 37):
                ins, y = _inputs(kind, rows, dev, seed=rows), _targets(rows, dev, rows)
                grad, pred = _call(m, ins, y)
                ref, ref_pred = _helper(m, ins, y)
                tag = f'n={n} {kind} trainable={trainable} {readout} rows={rows}'
                print(f'{tag}: max|grad err|={np.abs(grad - ref).max():.2e} max|pred err|={np.abs(pred - ref_pred).max():.2e} '
                      f'max|grad|={np.abs(ref).max():.2e}')
                assert grad.shape == ref.shape
                np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL, err_msg=tag)
                np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL, err_msg=tag)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_noiseless_equals_ideal(dev, n, kind):
    from quanonet_amd import _lib
    for trainable in (True, False):
        for readout in READOUTS:
            m = _model(kind, n, trainable, readout, seed=n).to(dev)
            for rows in (1, 37, 1000):
                ins, y = _inputs(kind, rows, dev, seed=rows), _targets(rows, dev, rows)
                grad, pred = _call(m, ins, y, p=(0.0, 0.0, 0.0))
                flat = H.flat(m)
                ideal = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=dev)
                ipred = torch.zeros(rows, dtype=torch.float64, device=dev)
                _lib.model_loss_grad(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat, 1.0 / rows, ideal,
                                     ham_diag=_diag(m), pred=ipred)
                torch.cuda.synchronize()
                tag = f'n={n} {kind} trainable={trainable} {readout} rows={rows}'
                np.testing.assert_allclose(grad, ideal.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)
                np.testing.assert_allclose(pred, ipred.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)


@pytest.mark.parametrize('n,kind,readout', [(2, 'quanonet', 'Z'), (3, 'heaqnn', 'X'), (4, 'quanonet', 'diag'),
                                            (5, 'quanonet', 'Y'), (6, 'heaqnn', 'Z'), (5, 'heaqnn', 'diag')])
def test_pred_determinism_shards_batches(dev, n, kind, readout):
    from quanonet_amd import _lib
    m = _model(kind, n, True, readout, seed=3).to(dev)
    rows = 1000
    ins, y = _inputs(kind, rows, dev, seed=4), _targets(rows, dev, 4)
    grad, pred = _call(m, ins, y)
    # pred is the exact noisy forward's
    fwd, _ = _lib.model_forward_noisy_exact(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, H.flat(m), _noise().params(),
                                            ham_diag=_diag(m))
    torch.cuda.synchronize()
    np.testing.assert_allclose(pred, fwd.cpu().numpy(), rtol=0, atol=1e-13)
    # two calls, with and without pred: bitwise
    grad2, pred2 = _call(m, ins, y)
    grad3, _ = _call(m, ins, y, want_pred=False)
    assert np.array_equal(grad, grad2) and np.array_equal(pred, pred2) and np.array_equal(grad, grad3)
    # two shards with the global inv_batch_total add up to the whole batch
    cut = 389
    ga, pa = _call(m, tuple(t[:cut] for t in ins), y[:cut], inv=1.0 / rows)
    gb, pb = _call(m, tuple(t[cut:] for t in ins), y[cut:], inv=1.0 / rows)
    np.testing.assert_allclose(ga + gb, grad, rtol=0, atol=1e-12)
    assert np.array_equal(np.concatenate([pa, pb]), pred)
    # a row's pred does not depend on the batch it is in
    for chunk in (7, 64):
        for s in (0, 3 * chunk, rows - chunk):
            _, pc = _call(m, tuple(t[s:s + chunk] for t in ins), y[s:s + chunk])
            assert np.array_equal(pc, pred[s:s + chunk]), (chunk, s)


def _adam_state(flat):
    return flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)


@pytest.mark.parametrize('n,kind,readout,trainable', [(2, 'quanonet', 'Z', True), (5, 'quanonet', 'X', True),
                                                      (6, 'heaqnn', 'diag', True), (4, 'heaqnn', 'Y', False)])
def test_train_steps(dev, n, kind, readout, trainable):
    from quanonet_amd import _lib
    m = _model(kind, n, trainable, readout, seed=5).to(dev)
    bounds, sizes = H.schedule(37, steps=5, last=20)
    rows = bounds[-1]
    ins, y = _inputs(kind, rows, dev, seed=6), _targets(rows, dev, 6)
    desc, nz, diag = m.fused_desc(), _noise().params(), _diag(m)
    trunk = ins[1] if len(ins) > 1 else None
    lr, b1, b2, eps, wd = 3e-2, 0.9, 0.999, 1e-8, 0.0
    P = H.flat(m).numel()
    # one call
    p1, m1, v1 = _adam_state(H.flat(m))
    out1 = torch.zeros(5, P + 2, dtype=torch.float64, device=dev)
    _lib.model_train_steps_noisy_exact(desc, bounds, sizes, ins[0], trunk, y, p1, out1, m1, v1, 1, lr, b1, b2, eps, wd, nz,
                                       ham_diag=diag)
    # the loop of single calls
    p2, m2, v2 = _adam_state(H.flat(m))
    out2 = torch.zeros(5, P + 2, dtype=torch.float64, device=dev)
    for i in range(5):
        a, b = bounds[i], bounds[i + 1]
        _lib.model_loss_grad_noisy_exact(desc, ins[0][a:b], None if trunk is None else trunk[a:b], y[a:b], p2, nz, 1.0 / sizes[i],
                                         out2[i], ham_diag=diag)
        _lib.adam_step(p2, out2[i], m2, v2, i + 1, lr, b1, b2, eps, wd)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    assert not torch.equal(p1, H.flat(m))
    # five steps of torch.optim.Adam on the helper's gradients
    pt = H.flat(m).cpu().clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for i in range(5):
        a, b = bounds[i], bounds[i + 1]
        ref, _ = _helper(m, tuple(t[a:b] for t in ins), y[a:b], inv=1.0 / sizes[i], flat=pt.detach())
        np.testing.assert_allclose(out1[i].cpu().numpy(), ref, rtol=0, atol=1e-9, err_msg=f'step {i}')
        opt.zero_grad()
        pt.grad = torch.from_numpy(ref[:P].copy())
        opt.step()
    np.testing.assert_allclose(p1.cpu().numpy(), pt.detach().numpy(), rtol=0, atol=1e-9)


def test_errors_launch_nothing(dev):
    from quanonet_amd import _lib
    m = _model('quanonet', 3, True, 'Z').to(dev)
    ins, y = _inputs('quanonet', 10, dev), _targets(10, dev)
    desc, params = m.fused_desc(), H.flat(m)
    P = params.numel()
    state = lambda: (torch.full((P + 2,), 123.0, dtype=torch.float64, device=dev), torch.full((10,), 456.0, dtype=torch.float64, device=dev),
                     params.clone(), torch.full((P,), 7.0, dtype=torch.float64, device=dev), torch.full((P,), 8.0, dtype=torch.float64, device=dev))

    def untouched(st):
        torch.cuda.synchronize()
        g, pr, p, mm, vv = st
        return (torch.all(g == 123.0) and torch.all(pr == 456.0) and torch.equal(p, params) and torch.all(mm == 7.0)
                and torch.all(vv == 8.0))

    def both(d, i, exc, nz):
        st = state()
        g, pr, p, mm, vv = st
        out = torch.full((2, P + 2), 123.0, dtype=torch.float64, device=dev)
        with pytest.raises(exc):
            _lib.model_loss_grad_noisy_exact(d, i[0], i[1] if len(i) > 1 else None, y, p, nz, 0.1, g, pred=pr)
        with pytest.raises(exc):
            _lib.model_train_steps_noisy_exact(d, [0, 4, 10], [4, 6], i[0], i[1] if len(i) > 1 else None, y, p, out, mm, vv, 1,
                                               1e-2, 0.9, 0.999, 1e-8, 0.0, nz)
        assert untouched(st) and torch.all(out == 123.0)

    for bad in (_lib.NoiseParams(-0.01, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.5, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
                _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0)):
        both(desc, ins, _lib.QheaError, bad)
    # the guard: a singular channel, and rates whose amplification over this circuit exceeds 10^12
    for nz in (_lib.NoiseParams(0.75, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 15 / 16, 0, 0, 1, 0), _lib.NoiseParams(0.6, 0.8, 0, 0, 1, 0)):
        assert not _lib.model_exact_noisy_log10_amplification(desc, nz) <= 12.0
        both(desc, ins, _lib.Unsupported, nz)
    m7 = _model('heaqnn', 7, True, 'Z').to(dev)
    ins7 = _inputs('heaqnn', 10, dev)
    p7 = H.flat(m7)
    g7 = torch.full((p7.numel() + 2,), 123.0, dtype=torch.float64, device=dev)
    pr7 = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.Unsupported):
        _lib.model_loss_grad_noisy_exact(m7.fused_desc(), ins7[0], None, y, p7, _noise().params(), 0.1, g7, pred=pr7)
    torch.cuda.synchronize()
    assert torch.all(g7 == 123.0) and torch.all(pr7 == 456.0)


def test_graph_capture_three_launches_per_step(dev):
    from quanonet_amd import _lib
    m = _model('quanonet', 5, True, 'Z').to(dev)
    bounds, sizes = H.schedule(100, steps=3, last=60)
    ins, y = _inputs('quanonet', bounds[-1], dev), _targets(bounds[-1], dev)
    desc, nz = m.fused_desc(), _noise().params()
    P = H.flat(m).numel()

    def run(st):
        p, mm, vv, out = st
        _lib.model_train_steps_noisy_exact(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0, nz)

    fresh = lambda: (*_adam_state(H.flat(m)), torch.zeros(3, P + 2, dtype=torch.float64, device=dev))
    eager = fresh()
    run(eager)                                                                     # also sizes the workspace outside the capture
    torch.cuda.synchronize()
    scratch = fresh()
    names = [k[0] for k in H.kernel_launches(dev, lambda: run(scratch))]
    assert len(names) == 9, names
    for i in range(3):
        step = names[3 * i:3 * i + 3]
        for k, kernel in enumerate(('prep_model_kernel', 'density_bwd_kernel', 'reduce_density_kernel')):
            assert kernel in step[k], (i, k, step)
    # a captured graph, replayed on fresh state, gives the eager result bitwise
    st = fresh()
    s = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run(st)
    for t, src in zip(st, fresh()):
        t.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(st, eager):
        assert torch.equal(a, b)


def test_python_api(dev):
    from quanonet_amd.noise import amplification, exact_noisy_loss_and_grad
    m = _model('quanonet', 4, True, 'X', seed=2).to(dev)
    ins, y = _inputs('quanonet', 37, dev, seed=2), _targets(37, dev, 2)
    got = exact_noisy_loss_and_grad(m, ins, y.reshape(-1, 1), _noise())
    torch.cuda.synchronize()
    ref, _ = _helper(m, ins, y)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=ATOL)
    from oracle import hea_oracle as O
    assert abs(amplification(m, _noise()) - DG.log10_amplification(4, O.block_configs_quanonet(4, m.net_size), P3[0], P3[1])) < 1e-12


def _cfg(tmp_path, name, **kw):
    cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': 2, 'net_size': [2, 1, 2, 1], 'scale_coeff': 0.5,
           'if_trainable_freq': 'true', 'learning_rate': 2e-2, 'batch_size': 100, 'num_epochs': 6, 'seed': 0,
           'prefix': str(tmp_path / name), 'run_id': 'r0', 'eval_batch_size': 64, 'trace_steps': True}
    cfg.update(kw)
    return cfg


def test_ptsolver_train_noise(dev, tmp_path):
    from quanonet_amd.noise import NoiseModel, exact_noisy_predict
    from quanonet_amd.solver import PTSolver, regression_metrics, set_random_seed
    data = _solver_data()
    nz = NoiseModel(p1=0.02, p2=0.05, readout=0.03)
    lines = []
    set_random_seed(0)
    s = PTSolver(_cfg(tmp_path, 'aware', train_noise=nz.asdict()), data, device=dev, log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    assert s.trainer.train_noise == nz
    assert sum('noise-aware training' in ln for ln in lines) == 1
    start = H.flat(s.model).cpu().clone()
    spec = DG.spec_of(s.model)
    hist = s.train()
    # the first steps over the traced row order: a host loop of the helper + torch Adam
    idx = np.asarray(hist['indices'][0])
    pt = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=2e-2)
    P = pt.numel()
    for i in range(3):
        rows = idx[100 * i:100 * (i + 1)]
        ref, _ = DG.model_loss_grad(spec, pt.detach().numpy(), data['train_branch_input'][rows], data['train_trunk_input'][rows],
                                    data['train_output'][rows, 0], nz.p1, nz.p2, nz.readout, 1.0 / 100)
        assert abs(hist['loss_steps'][i] - ref[P] / 100) < 1e-9, i
        opt.zero_grad()
        pt.grad = torch.from_numpy(ref[:P].copy())
        opt.step()
    assert hist['loss_train'][-1] < hist['loss_train'][0]
    # metric.json is the ideal score; evaluate_noisy(exact=True) the matching noisy one
    s.evaluate(hist)
    with open(os.path.join(s.out_dir, 'metric.json')) as f:
        metric = json.load(f)
    y_true = torch.tensor(data['test_output'], device=dev)
    ideal = regression_metrics(s.predict(s.test_input), y_true)
    assert metric['metrics']['MSE'] == ideal['MSE']
    res = s.evaluate_noisy(nz, exact=True)
    pred, _ = exact_noisy_predict(s.model, s.test_input, nz)
    assert res['MSE'] == regression_metrics(pred, y_true)['MSE'] and res['MSE'] != ideal['MSE']
    # one host call per step gives the same run
    set_random_seed(0)
    s2 = PTSolver(_cfg(tmp_path, 'aware_steps', train_noise=nz, epoch_call=False), data, device=dev, log=lambda *a, **k: None)
    h2 = s2.train()
    assert h2['loss_steps'] == hist['loss_steps']
    # a config without the key takes the ideal path
    set_random_seed(0)
    s3 = PTSolver(_cfg(tmp_path, 'ideal'), data, device=dev, log=lambda *a, **k: None)
    assert s3.trainer.train_noise is None
    assert s3.train()['loss_steps'][0] != hist['loss_steps'][0]
    with pytest.raises(ValueError):
        PTSolver(_cfg(tmp_path, 'bad', train_noise={'p1': 0.75}), data, device=dev, log=lambda *a, **k: None)
    with pytest.raises(ValueError):
        PTSolver(_cfg(tmp_path, 'bad2', train_noise=0.1), data, device=dev, log=lambda *a, **k: None)


def test_sweep_solvers_refuse_train_noise(dev, tmp_path):
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    from quanonet_amd.sweep import SweepSolver
    data = _solver_data()
    quiet = lambda *a, **k: None
    for cls in (EnsembleSolver, SweepSolver, DepthSweepSolver, QubitSweepSolver):
        cfgs = [_cfg(tmp_path, cls.__name__, seed=k, run_id=f'm{k}') for k in (0, 1)]
        cfgs[1]['train_noise'] = {'p1': 0.01}
        with pytest.raises(ValueError, match='train_noise'):
            cls(cfgs, data, device=dev, log=quiet)
