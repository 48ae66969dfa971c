"""
Exact noise-aware training at n = 7..9 on the GPU (qhea_model_loss_grad_noisy_exact_wide /
qhea_model_train_steps_noisy_exact_wide, quanonet_amd.noise.wide_exact_noisy_loss_and_grad, DataParallelTrainer / PTSolver with
train_noise_exact='wide') against the numpy helper tests/density_grad_reference.py (inverse walk, n-generic): the whole [P + 2]
buffer and pred, noiseless = the ideal call, pred bitwise the tiled exact forward's, shards, train_steps = the loop of single
calls, errors, the launch count of the header, the Python API.  Tolerance against the helper: atol 1e-10, as for n <= 6.
The shapes are the smallest that reach every stage map: every n has a block without sub-layers (the one-qubit stages A and B)
and a first sub-layer with its encoding (ring stages A and B), 1..3 rows.
"""
import numpy as np
import pytest
import torch

from tests import density_grad_reference as DG
from tests import helpers as H
from tests.test_noisy_forward import _inputs, _solver_data

pytestmark = pytest.mark.gpu
ATOL = 1e-10
P3 = (0.03, 0.08, 0.04)
WORST = {'grad': 0.0, 'pred': 0.0}


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


def _model(kind, n, trainable, readout, seed=0):
    """fp64 model on the CPU.  'quanonet': net (2, 0, 1, 2), two blocks without sub-layers and one block of two sub-layers
    (a first sub-layer with its encoding, one without); 'heaqnn': net (3, 1), three blocks of one sub-layer"""
    kw = dict(if_trainable_freq=trainable, scale_coeff=0.7, ham_bound=(-2.0, 3.0))
    if readout == 'diag':
        kw['ham_diag'] = np.random.default_rng(seed + 50).normal(size=1 << n)
    else:
        kw['ham_pauli'] = readout
    m = H.quanonet(n, 3, 2, (2, 0, 1, 2), seed, **kw) if kind == 'quanonet' else H.heaqnn(n, 4, (3, 1), seed, **kw)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(seed + 7)
        for name, p in m.named_parameters():
            if name.endswith('freq.weights'):
                p.copy_(0.5 + torch.rand(p.shape, generator=gen, dtype=torch.float64))
    return m


def _call(m, ins, y, p=P3, inv=None, want_pred=True, flat=None):
    """(grad[P+2], pred[B]) of one qhea_model_loss_grad_noisy_exact_wide call as numpy arrays"""
    from quanonet_amd import _lib
    flat = H.flat(m) if flat is None else flat
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device) if want_pred else None
    _lib.model_loss_grad_noisy_exact_wide(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat, _noise(p).params(),
                                          1.0 / rows if inv is None else inv, grad, ham_diag=_diag(m), pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (pred.cpu().numpy() if want_pred else None)


def _helper(m, ins, y, p=P3, inv=None):
    rows = ins[0].shape[0]
    return DG.model_loss_grad(DG.spec_of(m), H.flat(m).cpu().numpy(), ins[0].cpu().numpy(),
                              ins[1].cpu().numpy() if len(ins) > 1 else None, y.cpu().numpy(), *p,
                              1.0 / rows if inv is None else inv, inverse=True)


HELPER_CASES = ([(7, kind, trainable, readout, (1, 3)) for kind in ('quanonet', 'heaqnn') for trainable in (True, False)
                 for readout in ('Z', 'X', 'Y', 'diag')]
                + [(8, kind, True, readout, (3,)) for kind in ('quanonet', 'heaqnn') for readout in ('Z', 'diag')]
                + [(9, 'quanonet', True, 'Y', (2,)), (9, 'heaqnn', True, 'diag', (2,))])


@pytest.mark.parametrize('n,kind,trainable,readout,row_counts', HELPER_CASES)
def test_against_the_helper(dev, n, kind, trainable, readout, row_counts):
    m = _model(kind, n, trainable, readout, seed=n).to(dev)
    for rows in row_counts:
        ins, y = _inputs(kind, rows, dev, seed=rows), _targets(rows, dev, rows)
        grad, pred = _call(m, ins, y)
        ref, ref_pred = _helper(m, ins, y)
        tag = f'n={n} {kind} trainable={trainable} {readout} rows={rows}'
        ge, pe = np.abs(grad - ref).max(), np.abs(pred - ref_pred).max()
        WORST['grad'], WORST['pred'] = max(WORST['grad'], ge), max(WORST['pred'], pe)
        print(f"{tag}: max|grad err|={ge:.2e} max|pred err|={pe:.2e} max|grad|={np.abs(ref).max():.2e} "
              f"(largest so far: grad {WORST['grad']:.2e}, pred {WORST['pred']:.2e})")
        assert grad.shape == ref.shape
        np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL, err_msg=tag)
        np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL, err_msg=tag)


@pytest.mark.parametrize('n', [7, 8, 9])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_noiseless_equals_ideal(dev, n, kind):
    """the check at a batch no numpy walk reaches: at p = 0 the buffer is the ideal call's"""
    from quanonet_amd import _lib
    readout = 'diag' if kind == 'heaqnn' else {7: 'X', 8: 'Y', 9: 'Z'}[n]
    m = _model(kind, n, True, readout, seed=n).to(dev)
    flat = H.flat(m)
    for rows in (1, 5, 70):
        ins, y = _inputs(kind, rows, dev, seed=rows), _targets(rows, dev, rows)
        grad, pred = _call(m, ins, y, p=(0.0, 0.0, 0.0))
        ideal = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=dev)
        ipred = torch.zeros(rows, dtype=torch.float64, device=dev)
        _lib.model_loss_grad(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat, 1.0 / rows, ideal,
                             ham_diag=_diag(m), pred=ipred)
        torch.cuda.synchronize()
        tag = f'n={n} {kind} {readout} rows={rows}'
        np.testing.assert_allclose(grad, ideal.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)
        np.testing.assert_allclose(pred, ipred.cpu().numpy(), rtol=0, atol=ATOL, err_msg=tag)


@pytest.mark.parametrize('n,kind,readout,rows,cuts', [(7, 'quanonet', 'Y', 37, (13,)), (8, 'heaqnn', 'Z', 11, (1, 4)),
                                                      (9, 'heaqnn', 'diag', 7, (3,))])
def test_pred_bitwise_and_shards(dev, n, kind, readout, rows, cuts):
    from quanonet_amd import _lib
    m = _model(kind, n, True, readout, seed=3).to(dev)
    ins, y = _inputs(kind, rows, dev, seed=4), _targets(rows, dev, 4)
    grad, pred = _call(m, ins, y)
    # pred is the tiled exact forward's, bit for bit
    fwd, _ = _lib.model_forward_noisy_exact_wide(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, H.flat(m),
                                                 _noise().params(), ham_diag=_diag(m))
    torch.cuda.synchronize()
    assert np.array_equal(pred, fwd.cpu().numpy())
    # two calls, with and without pred: bitwise
    grad2, pred2 = _call(m, ins, y)
    grad3, _ = _call(m, ins, y, want_pred=False)
    assert np.array_equal(grad, grad2) and np.array_equal(pred, pred2) and np.array_equal(grad, grad3)
    # shards of uneven size with the global inv_batch_total: pred bitwise, the buffers add up to the whole call's
    bounds = (0,) + tuple(cuts) + (rows,)
    total, preds = 0.0, []
    for a, b in zip(bounds[:-1], bounds[1:]):
        g, p = _call(m, tuple(t[a:b] for t in ins), y[a:b], inv=1.0 / rows)
        total = total + g
        preds.append(p)
    assert np.array_equal(np.concatenate(preds), pred)
    np.testing.assert_allclose(total, grad, rtol=0, atol=1e-12)


def _adam_state(flat):
    return flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)


@pytest.mark.parametrize('n,kind,readout,trainable', [(7, 'quanonet', 'X', True), (8, 'heaqnn', 'diag', False)])
def test_train_steps(dev, n, kind, readout, trainable):
    """three steps with uneven bounds = the Python loop of loss_grad + adam_step, bitwise in parameters, moments and rows"""
    from quanonet_amd import _lib
    m = _model(kind, n, trainable, readout, seed=5).to(dev)
    bounds, sizes = [0, 5, 7, 14], [5, 2, 7]
    rows = bounds[-1]
    ins, y = _inputs(kind, rows, dev, seed=6), _targets(rows, dev, 6)
    desc, nz, diag = m.fused_desc(), _noise().params(), _diag(m)
    trunk = ins[1] if len(ins) > 1 else None
    lr, b1, b2, eps, wd = 3e-2, 0.9, 0.999, 1e-8, 0.0
    P = H.flat(m).numel()
    p1, m1, v1 = _adam_state(H.flat(m))
    out1 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
    _lib.model_train_steps_noisy_exact_wide(desc, bounds, sizes, ins[0], trunk, y, p1, out1, m1, v1, 1, lr, b1, b2, eps, wd, nz,
                                            ham_diag=diag)
    p2, m2, v2 = _adam_state(H.flat(m))
    out2 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
    for i in range(3):
        a, b = bounds[i], bounds[i + 1]
        _lib.model_loss_grad_noisy_exact_wide(desc, ins[0][a:b], None if trunk is None else trunk[a:b], y[a:b], p2, nz,
                                              1.0 / sizes[i], out2[i], ham_diag=diag)
        _lib.adam_step(p2, out2[i], m2, v2, i + 1, lr, b1, b2, eps, wd)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    assert not torch.equal(p1, H.flat(m))


def test_errors_launch_nothing(dev):
    from quanonet_amd import _lib
    m = _model('quanonet', 7, True, 'Z').to(dev)
    ins, y = _inputs('quanonet', 10, dev), _targets(10, dev)
    desc = m.fused_desc()

    def untouched(st, ref):
        torch.cuda.synchronize()
        g, pr, p, mm, vv = st
        return (torch.all(g == 123.0) and torch.all(pr == 456.0) and torch.equal(p, ref) and torch.all(mm == 7.0)
                and torch.all(vv == 8.0))

    def both(mod, kind, exc, nz):
        d, i, ref = mod.fused_desc(), _inputs(kind, 10, dev), H.flat(mod)
        Pm = ref.numel()
        g = torch.full((Pm + 2,), 123.0, dtype=torch.float64, device=dev)
        pr = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
        p, mm, vv = ref.clone(), torch.full((Pm,), 7.0, dtype=torch.float64, device=dev), torch.full((Pm,), 8.0, dtype=torch.float64, device=dev)
        out = torch.full((2, Pm + 2), 123.0, dtype=torch.float64, device=dev)
        trunk = i[1] if len(i) > 1 else None
        with pytest.raises(exc):
            _lib.model_loss_grad_noisy_exact_wide(d, i[0], trunk, y, p, nz, 0.1, g, pred=pr)
        with pytest.raises(exc):
            _lib.model_train_steps_noisy_exact_wide(d, [0, 4, 10], [4, 6], i[0], trunk, y, p, out, mm, vv, 1, 1e-2, 0.9, 0.999,
                                                    1e-8, 0.0, nz)
        assert untouched((g, pr, p, mm, vv), ref) and torch.all(out == 123.0)

    for bad in (_lib.NoiseParams(-0.01, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.5, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
                _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0)):
        both(m, 'quanonet', _lib.QheaError, bad)
    # the guard: a singular channel, and rates whose amplification over this circuit exceeds 10^12
    for nz in (_lib.NoiseParams(0.75, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 15 / 16, 0, 0, 1, 0), _lib.NoiseParams(0.6, 0.8, 0, 0, 1, 0)):
        assert not _lib.model_exact_noisy_log10_amplification(desc, nz) <= 12.0
        both(m, 'quanonet', _lib.Unsupported, nz)
    # the qubit counts on either side of the range
    for n in (6, 10):
        mo = _model('heaqnn', n, True, 'Z').to(dev)
        both(mo, 'heaqnn', _lib.Unsupported, _noise().params())
        g = torch.full((H.flat(mo).numel() + 2,), 123.0, dtype=torch.float64, device=dev)
        with pytest.raises(_lib.Unsupported, match='7..9'):           # the message names the range
            _lib.model_loss_grad_noisy_exact_wide(mo.fused_desc(), _inputs('heaqnn', 10, dev)[0], None, y, H.flat(mo),
                                                  _noise().params(), 0.1, g)
        torch.cuda.synchronize()
        assert torch.all(g == 123.0)


def _is_kernel(name, ident, n=None):
    """whether a mangled kernel name is `ident` of a unit's unnamed namespace, with first template argument n where given"""
    return f'_GLOBAL__N_1{len(ident)}{ident}' + ('' if n is None else f'ILi{n}E') in name


@pytest.mark.parametrize('n', [7, 9])
def test_graph_capturable_launch_count(dev, n):
    """the header's count, 6 + 4 (S + Z + R) launches per step, for a model with blocks without sub-layers and an X read-out;
    the captured graph replays to the eager result bitwise"""
    from quanonet_amd import _lib
    m = _model('quanonet', n, True, 'X').to(dev)                          # S = 2 sub-layers, Z = 2 empty blocks, R = 1
    S, Z, R = 2, 2, 1
    bounds, sizes = [0, 3, 5], [3, 2]
    ins, y = _inputs('quanonet', 5, dev), _targets(5, dev)
    desc, nz = m.fused_desc(), _noise().params()
    P = H.flat(m).numel()

    def run(st):
        p, mm, vv, out = st
        _lib.model_train_steps_noisy_exact_wide(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-2, 0.9, 0.999, 1e-8,
                                                0.0, nz)

    fresh = lambda: (*_adam_state(H.flat(m)), torch.zeros(2, P + 2, dtype=torch.float64, device=dev))
    eager = fresh()
    run(eager)                                                            # also sizes the workspace outside the capture
    torch.cuda.synchronize()
    scratch = fresh()
    launches = H.kernel_launches(dev, lambda: run(scratch))
    names = [k[0] for k in launches]
    per_step = 6 + 4 * (S + Z + R)
    assert len(names) == 2 * per_step, names
    for i, rows in enumerate(sizes):
        step = launches[per_step * i:per_step * (i + 1)]
        sn = [k[0] for k in step]
        assert 'prep_model_kernel' in sn[0] and 'density_wide_values_kernel' in sn[1], sn
        fwd = sn[2:2 + 2 * (S + Z + R)]
        assert sum(_is_kernel(k, 'density_wide_ring_kernel', n) for k in fwd) == 2 * S
        assert sum(_is_kernel(k, 'density_wide_wires_kernel', n) for k in fwd) == 2 * (Z + R)
        k0 = 2 + 2 * (S + Z + R)
        assert _is_kernel(sn[k0], 'density_wide_readout_kernel', n) and _is_kernel(sn[k0 + 1], 'density_wide_observable_kernel', n), sn
        back = sn[k0 + 2:-2]
        assert sum(_is_kernel(k, 'density_wide_ring_back_kernel', n) for k in back) == 2 * S
        assert sum(_is_kernel(k, 'density_wide_wires_back_kernel', n) for k in back) == 2 * (Z + R)
        assert len(back) == 2 * (S + Z + R)
        assert 'density_wide_fold_kernel' in sn[-2] and 'reduce_density_kernel' in sn[-1], sn
        for k in step:                                                    # every stage: one workgroup of 256 per (row, tile)
            if any(_is_kernel(k[0], ident, n) for ident in ('density_wide_ring_kernel', 'density_wide_wires_kernel',
                                                            'density_wide_ring_back_kernel', 'density_wide_wires_back_kernel',
                                                            'density_wide_observable_kernel')):
                assert k[1] == (rows * 4 ** (n - 6), 1, 1) and k[2] == (256, 1, 1), k
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
    from quanonet_amd.noise import DeviceNoise, exact_noisy_loss_and_grad, wide_exact_noisy_loss_and_grad
    m5 = _model('quanonet', 5, True, 'X', seed=2).to(dev)
    ins, y = _inputs('quanonet', 37, dev, seed=2), _targets(37, dev, 2)
    a = wide_exact_noisy_loss_and_grad(m5, ins, y.reshape(-1, 1), _noise())
    b = exact_noisy_loss_and_grad(m5, ins, y.reshape(-1, 1), _noise())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    m7 = _model('heaqnn', 7, True, 'Y', seed=2).to(dev)
    ins7, y7 = _inputs('heaqnn', 3, dev, seed=2), _targets(3, dev, 2)
    got = wide_exact_noisy_loss_and_grad(m7, ins7, y7.reshape(-1, 1), _noise())
    torch.cuda.synchronize()
    ref, _ = _helper(m7, ins7, y7)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=ATOL)
    shard = wide_exact_noisy_loss_and_grad(m7, ins7, y7, _noise(), inv_batch_total=0.5)
    np.testing.assert_allclose(shard.cpu().numpy()[:-2], 1.5 * ref[:-2], rtol=0, atol=ATOL)
    with pytest.raises(ValueError, match='device_trajectory_loss_and_grad'):
        wide_exact_noisy_loss_and_grad(m7, ins7, y7, DeviceNoise.uniform(_noise()))
    with pytest.raises(ValueError, match='sampled_noisy_loss_and_grad'):
        wide_exact_noisy_loss_and_grad(_model('heaqnn', 10, True, 'Z').to(dev), _inputs('heaqnn', 3, dev), y7, _noise())
    with pytest.raises(TypeError):
        wide_exact_noisy_loss_and_grad(torch.nn.Linear(2, 1), ins7, y7, _noise())


def _cfg(tmp_path, name, n=7, **kw):
    cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': n, 'net_size': [1, 1, 1, 0], 'scale_coeff': 0.5,
           'if_trainable_freq': 'true', 'learning_rate': 2e-2, 'batch_size': 100, 'num_epochs': 2, 'seed': 0,
           'prefix': str(tmp_path / name), 'run_id': 'r0', 'eval_batch_size': 64, 'trace_steps': True}
    cfg.update(kw)
    return cfg


def test_ptsolver_train_noise_exact_wide(dev, tmp_path):
    """n = 7: two epochs of three batches reproduce a manual loop of the calls over the traced row order"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import NoiseModel
    from quanonet_amd.solver import PTSolver, set_random_seed
    data = _solver_data()
    nz = NoiseModel(p1=0.02, p2=0.05, readout=0.03)
    quiet = lambda *a, **k: None
    lines = []
    set_random_seed(0)
    s = PTSolver(_cfg(tmp_path, 'wide', train_noise=nz.asdict(), train_noise_exact='wide'), data, device=dev,
                 log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    assert s.trainer.train_noise == nz and s.trainer.train_noise_exact == 'wide' and s.trainer.peer_fused is False
    start = H.flat(s.model).clone()
    desc, diag = s.model.fused_desc(), _diag(s.model)
    hist = s.train()
    # said once, at the first step, with the workspace of the configured batch
    said = [ln for ln in lines if 'noise-aware training' in ln]
    mib = _lib.model_exact_noisy_wide_grad_workspace_bytes(desc, 100) / 2 ** 20
    assert len(said) == 1 and 'exact noisy MSE' in said[0] and f'{mib:.1f} MiB for steps of up to 100 rows' in said[0], said
    assert len(hist['loss_steps']) == 6
    P = start.numel()
    branch, trunk = torch.tensor(data['train_branch_input'], device=dev), torch.tensor(data['train_trunk_input'], device=dev)
    target = torch.tensor(data['train_output'], device=dev).reshape(-1)
    p, mm, vv = _adam_state(start)
    buf = torch.zeros(P + 2, dtype=torch.float64, device=dev)
    step = 0
    for epoch in range(2):
        idx = torch.as_tensor(np.asarray(hist['indices'][epoch]), device=dev)
        for i in range(3):
            rows = idx[100 * i:100 * (i + 1)]
            _lib.model_loss_grad_noisy_exact_wide(desc, branch[rows].contiguous(), trunk[rows].contiguous(), target[rows].contiguous(),
                                                  p, nz.params(), 1.0 / 100, buf, ham_diag=diag)
            assert abs(hist['loss_steps'][step] - buf[P].item() / 100) < 1e-12, step
            step += 1
            _lib.adam_step(p, buf, mm, vv, step, 2e-2, 0.9, 0.999, 1e-8, 0.0)
    torch.cuda.synchronize()
    np.testing.assert_allclose(H.flat(s.model).cpu().numpy(), p.cpu().numpy(), rtol=0, atol=1e-12)
    assert not torch.equal(p, start)
    # one host call per step gives the same run
    set_random_seed(0)
    s2 = PTSolver(_cfg(tmp_path, 'wide_steps', train_noise=nz, train_noise_exact='wide', epoch_call=False), data, device=dev, log=quiet)
    assert s2.train()['loss_steps'] == hist['loss_steps']


def test_ptsolver_small_n_is_train_noise_alone(dev, tmp_path):
    """n = 5: the key changes nothing -- the run that train_noise alone describes, bitwise"""
    from quanonet_amd.noise import NoiseModel
    from quanonet_amd.solver import PTSolver, set_random_seed
    data = _solver_data()
    nz = NoiseModel(p1=0.02, p2=0.05, readout=0.03)
    quiet = lambda *a, **k: None
    runs = []
    for name, kw in (('alone', {}), ('wide', dict(train_noise_exact='wide'))):
        set_random_seed(0)
        s = PTSolver(_cfg(tmp_path, name, n=5, net_size=[2, 1, 2, 1], train_noise=nz.asdict(), **kw), data, device=dev, log=quiet)
        hist = s.train()
        runs.append((hist['loss_steps'], H.flat(s.model).clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


def test_refusals(dev, tmp_path):
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import DeviceNoise, NoiseModel, Sampling
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    from quanonet_amd.solver import DataParallelTrainer, PTSolver
    from quanonet_amd.sweep import SweepSolver
    data = _solver_data()
    quiet = lambda *a, **k: None
    nz = NoiseModel(p1=0.02, p2=0.05, readout=0.03)
    solver = lambda name, **kw: PTSolver(_cfg(tmp_path, name, **kw), data, device=dev, log=quiet)
    with pytest.raises(ValueError, match="None or 'wide'"):
        solver('value', train_noise=nz, train_noise_exact='tiled')
    with pytest.raises(ValueError, match='needs train_noise'):
        solver('alone', train_noise_exact='wide')
    dn = DeviceNoise.uniform(nz)
    with pytest.raises(ValueError, match='train_device_noise'):
        solver('device', train_device_noise=dn, train_noise_exact='wide')
    sp = Sampling(trajectories=8, seed=1)
    for key in ('train_sampling', 'train_trajectories'):
        with pytest.raises(ValueError, match=key):
            solver(key, train_noise=nz, train_noise_exact='wide', **{key: sp})
    with pytest.raises(ValueError, match='train_jump_trajectories'):
        solver('jump', train_noise=nz, train_noise_exact='wide', train_jump_trajectories=sp)
    with pytest.raises(ValueError, match='train_noise_states'):
        solver('states', train_noise=nz, train_noise_exact='wide', train_noise_states='stored')
    with pytest.raises(ValueError, match='n <= 9'):
        solver('n10', n=10, train_noise=nz, train_noise_exact='wide')
    with pytest.raises(ValueError, match='amplification'):                  # past the guard
        solver('guard', train_noise=NoiseModel(p1=0.6, p2=0.8), train_noise_exact='wide')
    # a non-fused model or optimizer
    m = _model('quanonet', 7, True, 'Z').to(dev)
    with pytest.raises(ValueError, match='fused'):
        DataParallelTrainer(m, fused=False, train_noise=nz, train_noise_exact='wide')
    with pytest.raises(ValueError, match='fused'):
        DataParallelTrainer(m, optimizer='sgd', train_noise=nz, train_noise_exact='wide')
    # train_noise alone at n = 7 still raises as before
    with pytest.raises(ValueError, match='n <= 6'):
        solver('plain7', train_noise=nz)
    # the four member solvers
    for cls in (EnsembleSolver, SweepSolver, DepthSweepSolver, QubitSweepSolver):
        cfgs = [_cfg(tmp_path, cls.__name__, n=2, net_size=[2, 1, 2, 1], seed=k, run_id=f'm{k}') for k in (0, 1)]
        cfgs[1]['train_noise_exact'] = 'wide'
        with pytest.raises(ValueError, match='train_noise_exact'):
            cls(cfgs, data, device=dev, log=quiet)
