"""
Training under the calibrated device noise model on the GPU (qhea_model_loss_grad_noisy_device_exact /
qhea_model_train_steps_noisy_device_exact, quanonet_amd.noise.device_noisy_loss_and_grad, DataParallelTrainer / PTSolver with
train_device_noise) against the numpy helper tests/device_noise_grad_reference.py (Kraus operators, slot by slot): the whole
[P + 2] buffer and pred for every shape, the reductions to the uniform and to the ideal call, pred = the exact device forward,
batch independence, train_steps = the loop of single calls, return codes, graph capture, the solvers.
Tolerance against the helper: atol 1e-10, the one the HIP path is held to everywhere.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import density_grad_reference as DG
from tests import device_noise_grad_reference as DV
from tests import helpers as H
from tests.test_device_noise_abi import BAD, _record
from tests.test_device_noise_training_abi import MAX_LOG10_AMPLIFICATION, as_dict, device_noise
from tests.test_noisy_forward import _inputs, _model, _solver_data

pytestmark = pytest.mark.gpu
ATOL = 1e-10
CASES = ((True, 'Z', True), (False, 'X', False), (True, 'Y', False), (False, 'diag', True))     # trainable, read-out, idle


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _targets(rows, dev, seed=0):
    return torch.tensor(np.random.default_rng(seed + 100).normal(scale=0.7, size=rows), device=dev)


def _diag(m):
    q = m.quantum_layer
    return q.ham_diag if q.use_full_ham else None


def _call(m, ins, y, dn, inv=None, want_pred=True, flat=None):
    """(grad[P+2], pred[B]) of one qhea_model_loss_grad_noisy_device_exact call as numpy arrays"""
    from quanonet_amd import _lib
    flat = H.flat(m) if flat is None else flat
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device) if want_pred else None
    _lib.model_loss_grad_noisy_device_exact(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat,
                                            dn.params(m.num_qubits), 1.0 / rows if inv is None else inv, grad,
                                            ham_diag=_diag(m), pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (pred.cpu().numpy() if want_pred else None)


def _helper(m, ins, y, dn, inv=None, flat=None):
    flat = H.flat(m) if flat is None else flat
    rows = ins[0].shape[0]
    return DV.model_loss_grad(DG.spec_of(m), flat.cpu().numpy(), ins[0].cpu().numpy(),
                              ins[1].cpu().numpy() if len(ins) > 1 else None, y.cpu().numpy(), as_dict(dn, m.num_qubits),
                              1.0 / rows if inv is None else inv)


def _check(m, kind, rows, dn, tag, dev, seed=None):
    ins, y = _inputs(kind, rows, dev, seed=rows if seed is None else seed), _targets(rows, dev, rows)
    grad, pred = _call(m, ins, y, dn)
    ref, ref_pred = _helper(m, ins, y, dn)
    print(f'{tag} rows={rows}: max|grad err|={np.abs(grad - ref).max():.2e} max|pred err|={np.abs(pred - ref_pred).max():.2e} '
          f'max|grad|={np.abs(ref).max():.2e}')
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL, err_msg=tag)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_against_the_helper(dev, n, kind):
    """sub-layers of depth 1 and 2; every wire's figures different, wire 1 without relaxation.  37 rows leave a tail slot in
    the last workgroup at n <= 4; at n = 5, 6 a workgroup is one row and 37 rows are 37 workgroups."""
    for k, (trainable, readout, idle) in enumerate(CASES):
        m = _model(kind, n, trainable, readout, seed=n).to(dev)
        dn = device_noise(n, idle, seed=k)
        tag = f'n={n} {kind} trainable={trainable} {readout} idle={idle}'
        _check(m, kind, 1, dn, tag, dev)
        _check(m, kind, 37, dn, tag, dev)


def test_two_workgroups_at_two_qubits(dev):
    """n = 2: a wave holds 64 rows, 65 rows are two workgroups"""
    for kind, (trainable, readout, idle) in (('quanonet', CASES[0]), ('heaqnn', CASES[3])):
        m = _model(kind, 2, trainable, readout, seed=2).to(dev)
        _check(m, kind, 65, device_noise(2, idle, seed=5), f'n=2 {kind} {readout}', dev)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
def test_blocks_without_sublayers(dev, n):
    """branch blocks of linear depth 0 (an encoding layer and its ENC sites only) behind a trunk block of depth 2"""
    for k, (readout, trainable, idle) in enumerate((('Z', True, True), ('Y', False, False))):
        m = H.quanonet(n, 3, 2, (2, 0, 1, 2), n, if_trainable_freq=trainable, scale_coeff=0.7, ham_bound=(-2.0, 3.0),
                       ham_pauli=readout).to(dev)
        for rows in (1, 37):
            _check(m, 'quanonet', rows, device_noise(n, idle, seed=7 + k), f'n={n} ld=0 {readout} idle={idle}', dev)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
def test_agreement_with_the_existing_calls(dev, n):
    """DeviceNoise.uniform(nz) = the uniform gradient call, DeviceNoise() = the ideal one, pred = the device forward's"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise, NoiseModel
    nz = NoiseModel(p1=0.03, p2=0.08, readout=0.04)
    rows = 37
    for kind, readout in (('quanonet', 'Z'), ('heaqnn', 'diag'), ('quanonet', 'X'), ('heaqnn', 'Y')):
        m = _model(kind, n, True, readout, seed=n).to(dev)
        ins, y = _inputs(kind, rows, dev, seed=rows), _targets(rows, dev, rows)
        trunk = ins[1] if len(ins) > 1 else None
        flat = H.flat(m)
        tag = f'n={n} {kind} {readout}'
        grad, pred = _call(m, ins, y, DeviceNoise.uniform(nz))
        want = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=dev)
        wpred = torch.zeros(rows, dtype=torch.float64, device=dev)
        _lib.model_loss_grad_noisy_exact(m.fused_desc(), ins[0], trunk, y, flat, nz.params(), 1.0 / rows, want, ham_diag=_diag(m),
                                         pred=wpred)
        torch.cuda.synchronize()
        print(f'{tag}: max|uniform diff|={np.abs(grad - want.cpu().numpy()).max():.2e}')
        np.testing.assert_allclose(grad, want.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)
        np.testing.assert_allclose(pred, wpred.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)
        grad, pred = _call(m, ins, y, DeviceNoise())
        _lib.model_loss_grad(m.fused_desc(), ins[0], trunk, y, flat, 1.0 / rows, want, ham_diag=_diag(m), pred=wpred)
        torch.cuda.synchronize()
        np.testing.assert_allclose(grad, want.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)
        np.testing.assert_allclose(pred, wpred.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)
        dn = device_noise(n, True, seed=3)
        grad, pred = _call(m, ins, y, dn)
        fwd, _ = _lib.model_forward_noisy_device_exact(m.fused_desc(), ins[0], trunk, flat, dn.params(n), ham_diag=_diag(m))
        torch.cuda.synchronize()
        print(f'{tag}: max|pred - device forward|={np.abs(pred - fwd.cpu().numpy()).max():.2e}')
        np.testing.assert_allclose(pred, fwd.cpu().numpy(), rtol=0, atol=1e-13, err_msg=tag)


@pytest.mark.parametrize('n,kind,readout', [(2, 'quanonet', 'Z'), (3, 'heaqnn', 'X'), (4, 'quanonet', 'diag'),
                                            (5, 'quanonet', 'Y'), (6, 'heaqnn', 'Z')])
def test_pred_is_batch_independent_and_calls_repeat(dev, n, kind, readout):
    m = _model(kind, n, True, readout, seed=3).to(dev)
    rows = 37
    dn = device_noise(n, True, seed=1)
    ins, y = _inputs(kind, rows, dev, seed=4), _targets(rows, dev, 4)
    grad, pred = _call(m, ins, y, dn)
    grad2, pred2 = _call(m, ins, y, dn)
    grad3, _ = _call(m, ins, y, dn, want_pred=False)
    assert np.array_equal(grad, grad2) and np.array_equal(pred, pred2) and np.array_equal(grad, grad3)
    for r in (0, 17, 36):                                                # a row alone is the row of the batch, bitwise
        _, p1 = _call(m, tuple(t[r:r + 1] for t in ins), y[r:r + 1], dn)
        assert p1[0] == pred[r], r
    # two shards with the global inv_batch_total add up to the whole batch
    ga, pa = _call(m, tuple(t[:13] for t in ins), y[:13], dn, inv=1.0 / rows)
    gb, pb = _call(m, tuple(t[13:] for t in ins), y[13:], dn, inv=1.0 / rows)
    np.testing.assert_allclose(ga + gb, grad, rtol=0, atol=1e-12)
    assert np.array_equal(np.concatenate([pa, pb]), pred)


def _adam_state(flat):
    return flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)


@pytest.mark.parametrize('n,kind,readout', [(3, 'quanonet', 'X'), (6, 'heaqnn', 'diag')])
def test_train_steps_is_the_loop_of_single_calls(dev, n, kind, readout):
    from quanonet_amd import _lib
    m = _model(kind, n, True, readout, seed=5).to(dev)
    bounds, sizes = H.schedule(37, steps=3, last=20)                     # ragged: the last step is shorter
    rows = bounds[-1]
    ins, y = _inputs(kind, rows, dev, seed=6), _targets(rows, dev, 6)
    desc, rec, diag = m.fused_desc(), device_noise(n, True, seed=2).params(n), _diag(m)
    trunk = ins[1] if len(ins) > 1 else None
    lr, b1, b2, eps, wd = 3e-2, 0.9, 0.999, 1e-8, 0.0
    P = H.flat(m).numel()
    p1, m1, v1 = _adam_state(H.flat(m))
    out1 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
    _lib.model_train_steps_noisy_device_exact(desc, bounds, sizes, ins[0], trunk, y, p1, out1, m1, v1, 1, lr, b1, b2, eps, wd,
                                              rec, ham_diag=diag)
    p2, m2, v2 = _adam_state(H.flat(m))
    out2 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
    for i in range(3):
        a, b = bounds[i], bounds[i + 1]
        _lib.model_loss_grad_noisy_device_exact(desc, ins[0][a:b], None if trunk is None else trunk[a:b], y[a:b], p2, rec,
                                                1.0 / sizes[i], out2[i], ham_diag=diag)
        _lib.adam_step(p2, out2[i], m2, v2, i + 1, lr, b1, b2, eps, wd)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    assert not torch.equal(p1, H.flat(m))


def test_errors_launch_nothing(dev):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    n = 5                                                                # the settings of BAD are written for five wires
    m = _model('quanonet', n, True, 'Z').to(dev)
    ins, y = _inputs('quanonet', 10, dev), _targets(10, dev)
    desc, params = m.fused_desc(), H.flat(m)
    P = params.numel()
    state = lambda: (torch.full((P + 2,), 123.0, dtype=torch.float64, device=dev),
                     torch.full((10,), 456.0, dtype=torch.float64, device=dev), params.clone(),
                     torch.full((P,), 7.0, dtype=torch.float64, device=dev), torch.full((P,), 8.0, dtype=torch.float64, device=dev))

    def untouched(st):
        torch.cuda.synchronize()
        g, pr, p, mm, vv = st
        return (torch.all(g == 123.0) and torch.all(pr == 456.0) and torch.equal(p, params) and torch.all(mm == 7.0)
                and torch.all(vv == 8.0))

    def both(d, i, yy, exc, rec):
        st = state()
        g, pr, p, mm, vv = st
        out = torch.full((2, P + 2), 123.0, dtype=torch.float64, device=dev)
        with pytest.raises(exc) as e1:
            _lib.model_loss_grad_noisy_device_exact(d, i[0], i[1] if len(i) > 1 else None, yy, p, rec, 0.1, g, pred=pr)
        with pytest.raises(exc) as e2:
            _lib.model_train_steps_noisy_device_exact(d, [0, 4, 10], [4, 6], i[0], i[1] if len(i) > 1 else None, yy, p, out, mm,
                                                      vv, 1, 1e-2, 0.9, 0.999, 1e-8, 0.0, rec)
        if exc is _lib.QheaError:                                        # QHEA_EINVAL, not its subclass for QHEA_EUNSUPPORTED
            assert not isinstance(e1.value, _lib.Unsupported) and not isinstance(e2.value, _lib.Unsupported)
        assert untouched(st) and torch.all(out == 123.0)

    for over in BAD:
        both(desc, ins, y, _lib.QheaError, _record(n, **over))
    # the guard: singular rates, and a long t_cx whose decay the inverse walk would have to undo
    ok = dict(p1=[0.01] * n, p2=[0.02] * n, t1=[1.0] * n, t2=[1.5] * n, t_rx=0.01, t_rot=0.02, t_cx=0.03)
    for over in (dict(p1=[0.01, 0.75, 0.01, 0.01, 0.01]), dict(p2=[15 / 16, 0.02, 0.02, 0.02, 0.02]), dict(t_cx=5.0),
                 dict(t_cx=1e4)):
        rec = DeviceNoise(**dict(ok, **over)).params(n)
        assert not _lib.model_device_noisy_log10_amplification(desc, rec) <= MAX_LOG10_AMPLIFICATION
        both(desc, ins, y, _lib.Unsupported, rec)
    m7 = _model('heaqnn', 7, True, 'Z').to(dev)
    ins7 = _inputs('heaqnn', 10, dev)
    p7 = H.flat(m7)
    g7 = torch.full((p7.numel() + 2,), 123.0, dtype=torch.float64, device=dev)
    pr7 = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.Unsupported):
        _lib.model_loss_grad_noisy_device_exact(m7.fused_desc(), ins7[0], None, y, p7, _record(7), 0.1, g7, pred=pr7)
    torch.cuda.synchronize()
    assert torch.all(g7 == 123.0) and torch.all(pr7 == 456.0)


@pytest.mark.parametrize('n', [2, 5])
def test_workspace_size_and_empty_batch(dev, n):
    """a workspace of exactly qhea_model_device_noisy_grad_workspace_bytes is accepted, one byte fewer is refused with the
    outputs untouched; an empty batch returns QHEA_OK"""
    from quanonet_amd import _lib
    lib = _lib.load()
    m = _model('quanonet', n, True, 'Z').to(dev)
    rows = 37
    ins, y = _inputs('quanonet', rows, dev), _targets(rows, dev)
    dn = device_noise(n, True)
    desc, params, rec = m.fused_desc(), H.flat(m), dn.params(n)
    want, want_pred = _call(m, ins, y, dn)
    need = int(lib.qhea_model_device_noisy_grad_workspace_bytes(ctypes.byref(desc), rows))
    assert 0 < need < (1 << 20)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    grad = torch.full((params.numel() + 2,), 123.0, dtype=torch.float64, device=dev)
    pred = torch.full((rows,), 456.0, dtype=torch.float64, device=dev)

    def call(batch, nbytes):
        with torch.cuda.device(dev):
            return lib.qhea_model_loss_grad_noisy_device_exact(ctypes.byref(desc), batch, _lib._ptr(ins[0]), _lib._ptr(ins[1]),
                                                               _lib._ptr(y), _lib._ptr(params), None, ctypes.byref(rec),
                                                               1.0 / rows, _lib._ptr(grad), _lib._ptr(pred), _lib._ptr(ws),
                                                               nbytes, _lib._stream(dev))
    assert call(rows, need - 1) == -3
    assert call(0, 0) == 0
    torch.cuda.synchronize()
    assert torch.all(grad == 123.0) and torch.all(pred == 456.0)
    assert call(rows, need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(grad.cpu().numpy(), want) and np.array_equal(pred.cpu().numpy(), want_pred)


@pytest.mark.parametrize('n', [2, 5, 6])
def test_graph_capture_three_launches_per_step(dev, n):
    from quanonet_amd import _lib
    m = _model('quanonet', n, True, 'Z').to(dev)
    bounds, sizes = H.schedule(37, steps=3, last=20)
    ins, y = _inputs('quanonet', bounds[-1], dev), _targets(bounds[-1], dev)
    desc, rec = m.fused_desc(), device_noise(n, True).params(n)
    P = H.flat(m).numel()

    def run(st):
        p, mm, vv, out = st
        _lib.model_train_steps_noisy_device_exact(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-2, 0.9, 0.999,
                                                  1e-8, 0.0, rec)

    fresh = lambda: (*_adam_state(H.flat(m)), torch.zeros(3, P + 2, dtype=torch.float64, device=dev))
    eager = fresh()
    run(eager)                                                           # also sizes the workspace outside the capture
    torch.cuda.synchronize()
    scratch = fresh()
    launches = H.kernel_launches(dev, lambda: run(scratch))
    names = [k[0] for k in launches]
    assert len(names) == 10, names                                       # the table kernel once, then three per step
    assert 'dev_table_kernel' in names[0] and launches[0][1] == (1, 1, 1), launches[0]
    for i in range(3):
        step = names[1 + 3 * i:4 + 3 * i]
        assert 'prep_model_kernel' in step[0] and 'reduce_density_kernel' in step[2], (i, step)
        assert f'density_dev_bwd_kernelILi{n}EE' in step[1], (i, step)
    threads = max(64, 1 << (2 * n - 4))
    rows_per_wg = threads >> (2 * n - 4)
    assert launches[2][1] == ((sizes[0] + rows_per_wg - 1) // rows_per_wg, 1, 1) and launches[2][2] == (threads, 1, 1), launches[2]
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
    from oracle import hea_oracle as O
    from quanonet_amd.noise import device_amplification, device_noisy_loss_and_grad
    n = 4
    m = _model('quanonet', n, True, 'X', seed=2).to(dev)
    dn = device_noise(n, True, seed=4)
    ins, y = _inputs('quanonet', 37, dev, seed=2), _targets(37, dev, 2)
    got = device_noisy_loss_and_grad(m, ins, y.reshape(-1, 1), dn)
    torch.cuda.synchronize()
    ref, _ = _helper(m, ins, y, dn)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=ATOL)
    half = device_noisy_loss_and_grad(m, ins, y, dn, inv_batch_total=0.5 / 37)
    np.testing.assert_allclose(half.cpu().numpy()[:-2], 0.5 * ref[:-2], rtol=0, atol=ATOL)
    want = DV.log10_amplification(n, O.block_configs_quanonet(n, m.net_size), as_dict(dn, n))
    assert abs(device_amplification(m, dn) - want) < 1e-12


def _cfg(tmp_path, name, **kw):
    cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': 2, 'net_size': [2, 1, 2, 1], 'scale_coeff': 0.5,
           'if_trainable_freq': 'true', 'learning_rate': 2e-2, 'batch_size': 100, 'num_epochs': 2, 'seed': 0,
           'prefix': str(tmp_path / name), 'run_id': 'r0', 'eval_batch_size': 64, 'trace_steps': True}
    cfg.update(kw)
    return cfg


def _solver_noise():
    from quanonet_amd.noise import DeviceNoise
    return DeviceNoise(p1=[0.01, 0.02], p2=[0.03, 0.02], readout01=[0.01, 0.02], readout10=[0.03, 0.04], t1=[1.0, math.inf],
                       t2=[1.5, 4.0], t_rx=0.01, t_rot=0.01, t_cx=0.05)


def test_ptsolver_train_device_noise(dev, tmp_path):
    from quanonet_amd.noise import NoiseModel, device_noisy_loss_and_grad, exact_noisy_predict
    from quanonet_amd.solver import PTSolver, regression_metrics, set_random_seed
    data = _solver_data()
    dn = _solver_noise()
    quiet = lambda *a, **k: None
    lines = []
    set_random_seed(0)
    s = PTSolver(_cfg(tmp_path, 'device', train_device_noise=dn.asdict()), data, device=dev,
                 log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    assert s.trainer.train_device_noise == dn and s.trainer.train_noise is None and s.trainer.peer_fused is False
    assert sum('device-noise training' in ln and 'log10 amplification' in ln for ln in lines) == 1
    start = H.flat(s.model).clone()
    hist = s.train()
    # the whole run over the traced row order: a hand loop of device_noisy_loss_and_grad + torch Adam
    ref_model = PTSolver(_cfg(tmp_path, 'hand'), data, device=dev, log=quiet).model
    with torch.no_grad():
        off = 0
        for p in ref_model.parameters():
            p.copy_(start[off:off + p.numel()].view(p.shape))
            off += p.numel()
    opt = torch.optim.Adam(ref_model.parameters(), lr=2e-2)
    P = start.numel()
    branch, trunk = torch.tensor(data['train_branch_input'], device=dev), torch.tensor(data['train_trunk_input'], device=dev)
    target = torch.tensor(data['train_output'], device=dev)
    step = 0
    for epoch in range(2):
        idx = torch.as_tensor(np.asarray(hist['indices'][epoch]), device=dev)
        for i in range(len(idx) // 100):
            rows = idx[100 * i:100 * (i + 1)]
            buf = device_noisy_loss_and_grad(ref_model, (branch[rows], trunk[rows]), target[rows], dn)
            assert abs(hist['loss_steps'][step] - buf[P].item() / 100) < 1e-9, step
            off = 0
            for p in ref_model.parameters():
                p.grad = buf[off:off + p.numel()].view(p.shape).clone()
                off += p.numel()
            opt.step()
            step += 1
    assert step == len(hist['loss_steps']) and step >= 4
    np.testing.assert_allclose(H.flat(s.model).cpu().numpy(), H.flat(ref_model).cpu().numpy(), rtol=0, atol=1e-9)
    assert hist['loss_train'][-1] < hist['loss_train'][0]
    # metric.json is the ideal score; evaluate_noisy(dn, exact=True) the matching one under the device
    s.evaluate(hist)
    with open(os.path.join(s.out_dir, 'metric.json')) as f:
        metric = json.load(f)
    y_true = torch.tensor(data['test_output'], device=dev)
    ideal = regression_metrics(s.predict(s.test_input), y_true)
    assert metric['metrics']['MSE'] == ideal['MSE']
    res = s.evaluate_noisy(dn, exact=True)
    pred, _ = exact_noisy_predict(s.model, s.test_input, dn)
    assert res['MSE'] == regression_metrics(pred, y_true)['MSE'] and res['MSE'] != ideal['MSE']
    # the ideal-trained model of the same seed under the device: reported, not asserted (two epochs of a toy fixture show no
    # ordering the numpy reference would vouch for)
    set_random_seed(0)
    s0 = PTSolver(_cfg(tmp_path, 'ideal'), data, device=dev, log=quiet)
    assert s0.trainer.train_device_noise is None
    h0 = s0.train()
    assert h0['loss_steps'][0] != hist['loss_steps'][0]
    print(f"MSE under the device: trained under it {res['MSE']:.6f}, trained ideal {s0.evaluate_noisy(dn, exact=True)['MSE']:.6f}")
    # one host call per step gives the same run
    set_random_seed(0)
    s2 = PTSolver(_cfg(tmp_path, 'device_steps', train_device_noise=dn, epoch_call=False), data, device=dev, log=quiet)
    assert s2.train()['loss_steps'] == hist['loss_steps']
    # refusals at construction
    for name, kw in (('both', dict(train_device_noise=dn, train_noise=NoiseModel(p1=0.01))),
                     ('both2', dict(train_device_noise=dn.asdict(), train_noise={'p1': 0.01})),
                     ('uniform', dict(train_noise=dn)), ('wrong', dict(train_device_noise=NoiseModel(p1=0.01))),
                     ('number', dict(train_device_noise=0.1)),
                     ('singular', dict(train_device_noise=dict(dn.asdict(), p1=[0.75, 0.01]))),
                     ('guard', dict(train_device_noise=dict(dn.asdict(), t_cx=20.0))),
                     ('wires', dict(train_device_noise=dict(dn.asdict(), p1=[0.01, 0.01, 0.01], p2=0.0, readout01=0.0,
                                                            readout10=0.0, t1=1.0, t2=1.0)))):
        with pytest.raises(ValueError):
            PTSolver(_cfg(tmp_path, name, **kw), data, device=dev, log=quiet)


def test_member_solvers_refuse_train_device_noise(dev, tmp_path):
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    from quanonet_amd.sweep import SweepSolver
    data = _solver_data()
    quiet = lambda *a, **k: None
    dn = _solver_noise().asdict()
    for cls in (EnsembleSolver, SweepSolver, DepthSweepSolver, QubitSweepSolver):
        cfgs = [_cfg(tmp_path, cls.__name__, seed=k, run_id=f'm{k}', train_device_noise=dn) for k in (0, 1)]
        with pytest.raises(ValueError, match='train_device_noise'):
            cls(cfgs, data, device=dev, log=quiet)
