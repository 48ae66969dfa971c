"""
Device-noise training from stored states on the GPU (qhea_model_loss_grad_noisy_device_exact_stored /
qhea_model_train_steps_noisy_device_exact_stored, device_noisy_loss_and_grad(states='stored'), PTSolver with
train_noise_states='stored') against the stored walk of the numpy helper tests/device_noise_grad_reference.py
(model_loss_grad(..., inverse=False)): inside the inverse walk's bound beside the inverse call, past it where that call refuses,
the headline shape once (120 units), a snapshot region past 4 GiB, and the bookkeeping (train_steps = the loop of single calls,
batch independence, workspace and guard refusals).  Tolerance against the helper: atol 1e-10 on the whole [P + 2] buffer.
tests/test_device_noise_stored_abi.py checks on the CPU that the settings past the bound are not vacuous.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import density_grad_reference as DG
from tests import device_noise_grad_reference as DV
from tests import helpers as H
from tests.test_device_noise_training_abi import MAX_LOG10_AMPLIFICATION, as_dict, device_noise, probe_setting

pytestmark = pytest.mark.gpu
ATOL = 1e-10
SHAPES = (('quanonet', (3, 2, 2, 1), True), ('heaqnn', (4, 3), False), ('quanonet', (2, 0, 1, 2), True))    # those of _shapes(n)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _shape_model(n, kind, net, trainable, readout, seed=0):
    """fp64 model on the CPU of one of the shapes of test_device_noise_training_abi._shapes; readout in 'Z', 'X', 'Y', 'diag'"""
    kw = dict(if_trainable_freq=trainable, scale_coeff=0.7, ham_bound=(-2.0, 3.0))
    if readout == 'diag':
        kw['ham_diag'] = np.random.default_rng(seed + 50).normal(size=1 << n)
    else:
        kw['ham_pauli'] = readout
    return H.quanonet(n, 4, 1, net, seed, **kw) if kind == 'quanonet' else H.heaqnn(n, 4, net, seed, **kw)


def _rows(kind, rows, seed):
    """(inputs, y) on the CPU"""
    rng = np.random.default_rng(seed)
    ins = (torch.tensor(rng.uniform(-1, 1, (rows, 4))),)
    if kind == 'quanonet':
        ins += (torch.tensor(rng.uniform(0, 1, (rows, 1))),)
    return ins, torch.tensor(rng.normal(scale=0.7, size=rows))


def _diag(m):
    q = m.quantum_layer
    return q.ham_diag if q.use_full_ham else None


def _call(m, ins, y, dn, states='stored', inv=None, flat=None):
    """(grad[P+2], pred[B]) of one loss_grad call as numpy arrays; the model and the rows are on the device"""
    from quanonet_amd import _lib
    flat = H.flat(m) if flat is None else flat
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device)
    call = _lib.model_loss_grad_noisy_device_exact_stored if states == 'stored' else _lib.model_loss_grad_noisy_device_exact
    call(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, y, flat, dn.params(m.num_qubits),
         1.0 / rows if inv is None else inv, grad, ham_diag=_diag(m), pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), pred.cpu().numpy()


def _helper(m, ins, y, dn):
    """the helper's stored walk: ([P + 2], pred)"""
    rows = ins[0].shape[0]
    return DV.model_loss_grad(DG.spec_of(m), H.flat(m).cpu().numpy(), ins[0].cpu().numpy(),
                              ins[1].cpu().numpy() if len(ins) > 1 else None, y.cpu().numpy(), as_dict(dn, m.num_qubits),
                              1.0 / rows, inverse=False)


def _to(dev, m, ins, y):
    return m.to(dev), tuple(t.to(dev) for t in ins), y.to(dev)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('shape', [0, 1, 2])
def test_inside_the_bound(dev, n, shape):
    """every shape of _shapes(n) -- depth 1, 2, 3 sub-layers, blocks without sub-layers, both models and frequency modes --
    against the helper's stored walk and against the inverse call.  37 rows leave a tail slot in the last workgroup at n <= 4;
    70 rows at n = 2 are two workgroups, the second with a tail.
    Three of the fifteen settings are not inside the inverse walk's bound -- log10 A_dev is 9.06 for the HEAQNN at n = 5, 7.58
    and 10.94 for the first two shapes at n = 6 -- so the inverse call refuses them, which is asserted; there the helper is the
    only reference for the buffer and pred is held to the exact device forward, to the 1e-13 it is held to beside the inverse
    call."""
    from quanonet_amd import _lib
    from quanonet_amd.noise import device_amplification
    kind, net, trainable = SHAPES[shape]
    dn = device_noise(n, idle=True)
    for readout in ('Z', 'Y') + (('X', 'diag') if n == 3 else ()):
        for rows in ((5,) if n == 6 else (1, 37) + ((70,) if n == 2 else ())):
            m = _shape_model(n, kind, net, trainable, readout, seed=n)
            inside = device_amplification(m, dn) <= MAX_LOG10_AMPLIFICATION
            assert inside == ((n, shape) not in ((5, 1), (6, 0), (6, 1)))
            ins, y = _rows(kind, rows, seed=10 * n + rows)
            m, ins, y = _to(dev, m, ins, y)
            grad, pred = _call(m, ins, y, dn)
            ref, ref_pred = _helper(m, ins, y, dn)
            tag = f'n={n} {kind} {net} {readout} rows={rows}'
            if inside:
                inv, inv_pred = _call(m, ins, y, dn, states='inverse')
            else:
                with pytest.raises(_lib.Unsupported):
                    _call(m, ins, y, dn, states='inverse')
                fwd, _ = _lib.model_forward_noisy_device_exact(m.fused_desc(), ins[0], ins[1] if len(ins) > 1 else None, H.flat(m),
                                                               dn.params(n), ham_diag=_diag(m))
                torch.cuda.synchronize()
                inv, inv_pred = ref, fwd.cpu().numpy()
            print(f'{tag}: max|grad - helper|={np.abs(grad - ref).max():.2e} max|pred - helper|={np.abs(pred - ref_pred).max():.2e} '
                  f'max|grad - inverse call|={np.abs(grad - inv).max():.2e} max|pred - inverse call|='
                  f'{np.abs(pred - inv_pred).max():.2e} max|grad|={np.abs(ref[:-2]).max():.2e}')
            assert grad.shape == ref.shape
            np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL, err_msg=tag)
            np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL, err_msg=tag)
            np.testing.assert_allclose(grad, inv, rtol=0, atol=ATOL, err_msg=tag)
            np.testing.assert_allclose(pred, inv_pred, rtol=0, atol=1e-13, err_msg=tag)


def past_the_bound_case(n, net, target, rows):
    """(spec, flat, x, y, DeviceNoise, log10 A_dev) of a fixed-frequency HEAQNN `net` on n qubits under the setting of the probe
    family with log10 A_dev = target; everything on the CPU (tests/test_device_noise_stored_abi.py walks it with the helper)"""
    m = past_the_bound_model(n, net)
    dn, logA = probe_setting(n, [(n, net[1])] * net[0], target)
    ins, y = _rows('heaqnn', rows, seed=100 * n + int(target))
    return DG.spec_of(m), H.flat(m).numpy(), ins[0].numpy(), y.numpy(), dn, logA


def past_the_bound_model(n, net):
    m = H.heaqnn(n, 4, net, n, if_trainable_freq=False, scale_coeff=0.7, ham_bound=(-2.0, 3.0))
    rng = np.random.default_rng(n)
    with torch.no_grad():                                                # angles all over the circle, as in the guard's probe
        w = m.quantum_layer.ansatz_weights
        w.copy_(torch.from_numpy(rng.uniform(-np.pi, np.pi, tuple(w.shape))))
    return m


@pytest.mark.parametrize('n,net,target,rows', [(3, (6, 2), 16.0, 3), (3, (6, 2), 20.0, 3), (5, (4, 2), 12.0, 1), (6, (3, 2), 12.0, 1)])
def test_past_the_bound(dev, n, net, target, rows):
    """log10 A_dev = 12, 16, 20: the inverse call refuses as it always did, the stored call matches the helper's stored walk,
    and the gradient it returns is not a vanishing one"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import device_amplification, device_layer_amplification
    spec, flat, x, y, dn, logA = past_the_bound_case(n, net, target, rows)
    m = past_the_bound_model(n, net)
    assert abs(device_amplification(m, dn) - target) < 1e-6 and device_layer_amplification(m, dn) <= MAX_LOG10_AMPLIFICATION
    m, ins, y = _to(dev, m, (torch.tensor(x),), torch.tensor(y))
    with pytest.raises(_lib.Unsupported):
        _call(m, ins, y, dn, states='inverse')
    grad, pred = _call(m, ins, y, dn)
    ref, ref_pred = _helper(m, ins, y, dn)
    print(f'n={n} net={net} log10 A_dev={logA:.2f} (layer {device_layer_amplification(m, dn):.2f}): max|grad - helper|='
          f'{np.abs(grad - ref).max():.2e} max|pred - helper|={np.abs(pred - ref_pred).max():.2e} '
          f'max|gradient|={np.abs(grad[:-2]).max():.2e}')
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL)
    assert np.abs(grad[:-2]).max() >= 1e-3


def test_headline_shape(dev):
    """Q5 Net40-2-20-2 under the rate scripts' device setting (log10 A_dev 10.99, refused by the inverse call): 120 units of
    snapshot indexing on 2 rows"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import device_amplification
    from scripts.device_noise_rate import device_noise as rate_noise
    n, rows = 5, 2
    m = H.quanonet(n, 100, 2, (40, 2, 20, 2), 0, if_trainable_freq=True, scale_coeff=0.1)
    dn = rate_noise(n)
    assert abs(device_amplification(m, dn) - 10.99) < 0.01
    rng = np.random.default_rng(5)
    ins = (torch.tensor(rng.normal(size=(rows, 100))), torch.tensor(rng.uniform(size=(rows, 2))))
    m, ins, y = _to(dev, m, ins, torch.tensor(rng.normal(scale=0.5, size=rows)))
    with pytest.raises(_lib.Unsupported):
        _call(m, ins, y, dn, states='inverse')
    grad, pred = _call(m, ins, y, dn)
    ref, ref_pred = _helper(m, ins, y, dn)
    print(f'Q5 Net40-2-20-2: max|grad - helper|={np.abs(grad - ref).max():.2e} max|pred - helper|={np.abs(pred - ref_pred).max():.2e} '
          f'max|gradient|={np.abs(ref[:-2]).max():.2e}')
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL)


def test_snapshots_past_4_gib(dev):
    """Q6 with 20 units at 3300 rows: 20 x 3300 x 64 KiB = 4.03 GiB of snapshots, so the last rows' offsets do not fit 32 bits.
    Inside the bound, against the inverse call: the last 64 rows' pred, and the buffer."""
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise, device_amplification
    n, rows = 6, 3300
    m = H.heaqnn(n, 4, (10, 2), 1, if_trainable_freq=True, scale_coeff=0.7, ham_bound=(-2.0, 3.0))
    dn = DeviceNoise(p1=[1e-3] * n, p2=[5e-3] * n, readout01=[0.01] * n, readout10=[0.02] * n, t1=[100.0] * n, t2=[80.0] * n,
                     t_rx=0.05, t_rot=0.05, t_cx=0.3)
    assert 1.0 < device_amplification(m, dn) <= MAX_LOG10_AMPLIFICATION
    snap = _lib.model_device_noisy_stored_grad_workspace_bytes(m.fused_desc(), rows) - int(
        _lib.load().qhea_model_device_noisy_grad_workspace_bytes(ctypes.byref(m.fused_desc()), rows))
    assert snap > 1 << 32
    ins, y = _rows('heaqnn', rows, seed=6)
    m, ins, y = _to(dev, m, ins, y)
    grad, pred = _call(m, ins, y, dn)
    inv, inv_pred = _call(m, ins, y, dn, states='inverse')
    print(f'Q6, 20 units, {rows} rows, {snap} snapshot bytes: max|grad - inverse call|={np.abs(grad - inv).max():.2e} '
          f'max|pred - inverse call| (last 64 rows)={np.abs(pred[-64:] - inv_pred[-64:]).max():.2e}')
    np.testing.assert_allclose(pred[-64:], inv_pred[-64:], rtol=0, atol=1e-13)
    np.testing.assert_allclose(grad, inv, rtol=0, atol=ATOL)
    assert np.abs(grad[:-2]).max() >= 1e-3


def _past_the_bound_on(dev, rows, seed=0):
    """a model past the total bound and inside the layer bound with its rows, on the device"""
    n, net = 3, (6, 2)
    m = past_the_bound_model(n, net)
    dn, _ = probe_setting(n, [(n, net[1])] * net[0], 16.0)
    ins, y = _rows('heaqnn', rows, seed=seed)
    return (*_to(dev, m, ins, y), dn)


def test_train_steps_is_the_loop_of_single_calls(dev):
    from quanonet_amd import _lib
    bounds, sizes = H.schedule(37, steps=3, last=20)                     # ragged: the last step is shorter
    m, ins, y, dn = _past_the_bound_on(dev, bounds[-1])
    desc, rec = m.fused_desc(), dn.params(3)
    lr, b1, b2, eps, wd = 3e-2, 0.9, 0.999, 1e-8, 0.0
    P = H.flat(m).numel()
    state = lambda: (H.flat(m).clone(), torch.zeros(P, dtype=torch.float64, device=dev), torch.zeros(P, dtype=torch.float64, device=dev),
                     torch.zeros(3, P + 2, dtype=torch.float64, device=dev))
    p1, m1, v1, out1 = state()
    _lib.model_train_steps_noisy_device_exact_stored(desc, bounds, sizes, ins[0], None, y, p1, out1, m1, v1, 1, lr, b1, b2, eps, wd, rec)
    p2, m2, v2, out2 = state()
    for i in range(3):
        a, b = bounds[i], bounds[i + 1]
        _lib.model_loss_grad_noisy_device_exact_stored(desc, ins[0][a:b], None, y[a:b], p2, rec, 1.0 / sizes[i], out2[i])
        _lib.adam_step(p2, out2[i], m2, v2, i + 1, lr, b1, b2, eps, wd)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    assert not torch.equal(p1, H.flat(m))
    with pytest.raises(_lib.Unsupported):
        _lib.model_train_steps_noisy_device_exact(desc, bounds, sizes, ins[0], None, y, p1, out1, m1, v1, 1, lr, b1, b2, eps, wd, rec)


@pytest.mark.parametrize('n', [3, 5])
def test_pred_does_not_depend_on_the_batch(dev, n):
    """37 rows called as 20 + 17 give bitwise the same pred (another grid, other slots, another snapshot stride), and the call
    repeats bitwise"""
    kind, net, trainable = SHAPES[2]
    m = _shape_model(n, kind, net, trainable, 'Y', seed=3)
    ins, y = _rows(kind, 37, seed=4)
    m, ins, y = _to(dev, m, ins, y)
    dn = device_noise(n, idle=True, seed=1)
    grad, pred = _call(m, ins, y, dn)
    grad2, pred2 = _call(m, ins, y, dn)
    assert np.array_equal(grad, grad2) and np.array_equal(pred, pred2)
    ga, pa = _call(m, tuple(t[:20] for t in ins), y[:20], dn, inv=1.0 / 37)
    gb, pb = _call(m, tuple(t[20:] for t in ins), y[20:], dn, inv=1.0 / 37)
    assert np.array_equal(np.concatenate([pa, pb]), pred)
    np.testing.assert_allclose(ga + gb, grad, rtol=0, atol=1e-12)


def test_refusals_leave_the_outputs_untouched(dev):
    """a workspace one byte short of qhea_model_device_noisy_stored_grad_workspace_bytes: QHEA_EWORKSPACE; a layer above the
    bound: QHEA_EUNSUPPORTED; the sentinels stay in both cases, and the exact size is accepted"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    lib = _lib.load()
    rows = 37
    m, ins, y, dn = _past_the_bound_on(dev, rows)
    desc, params = m.fused_desc(), H.flat(m)
    want, want_pred = _call(m, ins, y, dn)
    need = _lib.model_device_noisy_stored_grad_workspace_bytes(desc, rows)
    inverse_need = int(lib.qhea_model_device_noisy_grad_workspace_bytes(ctypes.byref(desc), rows))
    assert need == inverse_need + 12 * rows * 16 * 4 ** 3
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    grad = torch.full((params.numel() + 2,), 123.0, dtype=torch.float64, device=dev)
    pred = torch.full((rows,), 456.0, dtype=torch.float64, device=dev)

    def call(rec, nbytes):
        with torch.cuda.device(dev):
            return lib.qhea_model_loss_grad_noisy_device_exact_stored(ctypes.byref(desc), rows, _lib._ptr(ins[0]), None, _lib._ptr(y),
                                                                      _lib._ptr(params), None, ctypes.byref(rec), 1.0 / rows,
                                                                      _lib._ptr(grad), _lib._ptr(pred), _lib._ptr(ws), nbytes,
                                                                      _lib._stream(dev))
    above = DeviceNoise(p1=[0.01] * 3, p2=[0.02] * 3, t1=[1.0] * 3, t2=[1.5] * 3, t_rx=0.01, t_rot=0.02, t_cx=8.0)
    assert MAX_LOG10_AMPLIFICATION < _lib.model_device_noisy_log10_layer_amplification(desc, above.params(3)) < float('inf')
    assert call(dn.params(3), need - 1) == -3 and call(dn.params(3), inverse_need) == -3
    assert call(above.params(3), need) == -2
    torch.cuda.synchronize()
    assert torch.all(grad == 123.0) and torch.all(pred == 456.0)
    assert call(dn.params(3), need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(grad.cpu().numpy(), want) and np.array_equal(pred.cpu().numpy(), want_pred)


def test_ptsolver_train_noise_states(dev, tmp_path):
    """a small n = 3 model whose device_amplification is past 7: PTSolver with train_noise_states='stored' runs 3 steps that
    are device_noisy_loss_and_grad(states='stored') + torch Adam; without the key the constructor raises as it did"""
    from quanonet_amd.noise import DeviceNoise, device_amplification, device_layer_amplification, device_noisy_loss_and_grad
    from quanonet_amd.solver import PTSolver, set_random_seed
    from tests.test_noisy_forward import _solver_data
    data = _solver_data()
    dn = DeviceNoise(p1=[0.02, 0.03, 0.01], p2=[0.05, 0.04, 0.06], readout01=[0.01, 0.02, 0.01], readout10=[0.03, 0.04, 0.02],
                     t1=[1.0, float('inf'), 1.5], t2=[1.5, 4.0, 1.0], t_rx=0.04, t_rot=0.06, t_cx=0.2)

    def cfg(name, **kw):
        c = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': 3, 'net_size': [3, 2, 3, 2], 'scale_coeff': 0.5,
             'if_trainable_freq': 'true', 'learning_rate': 2e-2, 'batch_size': 100, 'num_epochs': 1, 'seed': 0,
             'prefix': str(tmp_path / name), 'run_id': 'r0', 'eval_batch_size': 64, 'trace_steps': True}
        c.update(kw)
        return c

    quiet = lambda *a, **k: None
    lines = []
    set_random_seed(0)
    s = PTSolver(cfg('stored', train_device_noise=dn.asdict(), train_noise_states='stored'), data, device=dev,
                 log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    amp, layer = device_amplification(s.model, dn), device_layer_amplification(s.model, dn)
    assert amp > MAX_LOG10_AMPLIFICATION > layer
    assert s.trainer.noise_states == 'stored' and s.trainer.train_device_noise == dn
    told = [ln for ln in lines if 'replayed from stored states' in ln]
    assert len(told) == 1 and f'{amp:.2f} in total' in told[0] and f'{layer:.2f} for one layer' in told[0]
    assert f'{12 * 16 * 4 ** 3} snapshot bytes per row' in told[0]
    start = H.flat(s.model).clone()
    hist = s.train()
    ref_model = PTSolver(cfg('hand'), data, device=dev, log=quiet).model
    with torch.no_grad():
        off = 0
        for p in ref_model.parameters():
            p.copy_(start[off:off + p.numel()].view(p.shape))
            off += p.numel()
    opt = torch.optim.Adam(ref_model.parameters(), lr=2e-2)
    P = start.numel()
    branch, trunk = torch.tensor(data['train_branch_input'], device=dev), torch.tensor(data['train_trunk_input'], device=dev)
    target = torch.tensor(data['train_output'], device=dev)
    idx = torch.as_tensor(np.asarray(hist['indices'][0]), device=dev)
    assert len(hist['loss_steps']) == 3 == len(idx) // 100
    for i in range(3):
        rows = idx[100 * i:100 * (i + 1)]
        buf = device_noisy_loss_and_grad(ref_model, (branch[rows], trunk[rows]), target[rows], dn, states='stored')
        assert abs(hist['loss_steps'][i] - buf[P].item() / 100) < 1e-9, i
        off = 0
        for p in ref_model.parameters():
            p.grad = buf[off:off + p.numel()].view(p.shape).clone()
            off += p.numel()
        opt.step()
    np.testing.assert_allclose(H.flat(s.model).cpu().numpy(), H.flat(ref_model).cpu().numpy(), rtol=0, atol=1e-9)
    assert not torch.equal(H.flat(s.model), start)
    # without the key (and with its default spelled out): refused at construction, as before
    for name, kw in (('none', {}), ('inverse', dict(train_noise_states='inverse'))):
        with pytest.raises(ValueError, match='the library refuses this model under this DeviceNoise'):
            PTSolver(cfg(name, train_device_noise=dn.asdict(), **kw), data, device=dev, log=quiet)
    with pytest.raises(ValueError, match="train_noise_states='stored': the library refuses"):
        PTSolver(cfg('layer', train_device_noise=dict(dn.asdict(), t_cx=20.0), train_noise_states='stored'), data, device=dev, log=quiet)
    from quanonet_amd import _lib
    with pytest.raises(_lib.Unsupported):
        device_noisy_loss_and_grad(ref_model, (branch[:5], trunk[:5]), target[:5], dn)
