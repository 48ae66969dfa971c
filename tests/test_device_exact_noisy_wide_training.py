"""
Exact device-noise training at n = 7..9 on the GPU (qhea_model_loss_grad_noisy_device_exact_wide /
qhea_model_train_steps_noisy_device_exact_wide, quanonet_amd.noise.device_exact_noisy_loss_and_grad, DataParallelTrainer /
PTSolver with train_device_noise_exact='wide') against the numpy helper tests/device_noise_grad_reference.py (inverse walk,
generic in n): the whole [P + 2] buffer and pred, the places where the device sites can go wrong and the uniform channels cannot,
the uniform setting = the uniform tiled call, the default setting = the ideal call, pred bitwise the tiled device forward's,
shards, train_steps = the loop of single calls, errors, the launch count of the header under graph capture, the Python API and
every refusal.  Tolerance against the helper: atol 1e-10, as everywhere.
The shapes are the smallest that reach every stage map: blocks of depth 0 (the reverse encoding stages A and B), 1 and 2 (ring
stages with and without the encoding), 1..3 rows; the helper's walk takes seconds per row at n = 9, so n = 8, 9 use one row.
"""
import math

import numpy as np
import pytest
import torch

from tests import density_grad_reference as DG
from tests import device_noise_grad_reference as DV
from tests import helpers as H
from tests.test_device_exact_noisy_wide import _net_model
from tests.test_device_noise_training_abi import as_dict, device_noise
from tests.test_exact_noisy_wide_training import _adam_state, _diag, _is_kernel, _model, _targets
from tests.test_noisy_forward import _inputs, _solver_data

pytestmark = pytest.mark.gpu
ATOL = 1e-10
WORST = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _trunk(ins):
    return ins[1] if len(ins) > 1 else None


def _call(m, ins, y, dn, inv=None, want_pred=True, flat=None):
    """(grad[P+2], pred[B]) of one qhea_model_loss_grad_noisy_device_exact_wide call as numpy arrays"""
    from quanonet_amd import _lib
    flat = H.flat(m) if flat is None else flat
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device) if want_pred else None
    _lib.model_loss_grad_noisy_device_exact_wide(m.fused_desc(), ins[0], _trunk(ins), y, flat, dn.params(m.num_qubits),
                                                 1.0 / rows if inv is None else inv, grad, ham_diag=_diag(m), pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (pred.cpu().numpy() if want_pred else None)


def _helper(m, ins, y, dn, inv=None):
    rows = ins[0].shape[0]
    return DV.model_loss_grad(DG.spec_of(m), H.flat(m).cpu().numpy(), ins[0].cpu().numpy(),
                              ins[1].cpu().numpy() if len(ins) > 1 else None, y.cpu().numpy(), as_dict(dn, m.num_qubits),
                              1.0 / rows if inv is None else inv, inverse=True)


def _against_helper(m, ins, y, dn, tag):
    grad, pred = _call(m, ins, y, dn)
    ref, ref_pred = _helper(m, ins, y, dn)
    n = m.num_qubits
    ge, pe = np.abs(grad - ref).max(), np.abs(pred - ref_pred).max()
    w = WORST.setdefault(n, {'grad': 0.0, 'pred': 0.0})
    w['grad'], w['pred'] = max(w['grad'], ge), max(w['pred'], pe)
    print(f"{tag}: max|grad err|={ge:.2e} max|pred err|={pe:.2e} max|grad|={np.abs(ref[:-2]).max():.2e} "
          f"(largest so far at n={n}: grad {w['grad']:.2e}, pred {w['pred']:.2e})")
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL, err_msg=tag)
    return grad, pred


# 'quanonet' (net (2, 0, 1, 2)): a block of two sub-layers and two without; 'heaqnn' (net (3, 1)): three blocks of one sub-layer
@pytest.mark.parametrize('readout', ['Z', 'X', 'Y', 'diag'])
@pytest.mark.parametrize('trainable', [True, False])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_against_the_helper_n7(dev, kind, trainable, readout):
    """the per-wire setting in which no two wires and no two slots agree and one wire has no relaxation (device_noise), idle on
    and off, 1 and 3 rows"""
    n = 7
    m = _model(kind, n, trainable, readout, seed=n).to(dev)
    for rows, idle in ((1, True), (1, False), (3, True), (3, False)):
        ins, y = _inputs(kind, rows, dev, seed=rows), _targets(rows, dev, rows)
        dn = device_noise(n, idle, seed=rows)
        _against_helper(m, ins, y, dn, f'n={n} {kind} trainable={trainable} {readout} rows={rows} idle={idle}')


@pytest.mark.parametrize('n,readout,idle', [(8, 'diag', True), (9, 'X', False)])
def test_against_the_helper_n8_n9(dev, n, readout, idle):
    """one row on the blocks (n, 1), (n, 0): a QuanONet of net (1, 0, 1, 1)"""
    from oracle import hea_oracle as O
    assert O.block_configs_quanonet(n, (1, 0, 1, 1)) == [(n, 1), (n, 0)]
    m = _net_model('quanonet', n, (1, 0, 1, 1), readout, seed=n).to(dev)
    ins, y = _inputs('quanonet', 1, dev, seed=n), _targets(1, dev, n)
    _against_helper(m, ins, y, device_noise(n, idle, seed=1), f'n={n} quanonet {readout} idle={idle}')


def _edge_setting(what, n):
    from quanonet_amd.noise import DeviceNoise
    inf = math.inf
    if what == 'closing-pair':                                           # relaxation on wires n - 1 and 0 alone
        return DeviceNoise(t1=(2.0,) + (inf,) * (n - 2) + (3.0,), t2=(1.5,) + (inf,) * (n - 2) + (4.0,), t_rx=0.05, t_rot=0.1,
                           t_cx=0.3, idle=True)
    if what == 'wire-6':                                                 # the first stage B wire: the map local + n - 6
        return DeviceNoise(t1=tuple(2.0 if q == 6 else inf for q in range(n)), t2=tuple(1.5 if q == 6 else inf for q in range(n)),
                           t_rx=0.05, t_rot=0.1, t_cx=0.3, idle=True)
    if what == 'readout-top-bit':                                        # asymmetric readout on bit n - 1 alone
        return DeviceNoise(readout01=(0.0,) * (n - 1) + (0.15,), readout10=(0.0,) * (n - 1) + (0.05,))
    assert what == 'p2-closing-slot'                                     # a p2 that differs on slot n - 1 alone
    return DeviceNoise(p2=(0.02,) * (n - 1) + (0.09,))


@pytest.mark.parametrize('what', ['closing-pair', 'wire-6', 'readout-top-bit', 'p2-closing-slot'])
@pytest.mark.parametrize('n', [7, 9])
def test_device_site_edges(dev, n, what):
    """where this kernel can go wrong and the uniform one cannot, each alone, on blocks (n, 1), (n, 0), one row"""
    m = _net_model('quanonet', n, (1, 0, 1, 1), 'Y' if what != 'readout-top-bit' else 'Z', seed=n + 2).to(dev)
    ins, y = _inputs('quanonet', 1, dev, seed=n + 1), _targets(1, dev, n + 1)
    dn = _edge_setting(what, n)
    grad, _ = _against_helper(m, ins, y, dn, f'n={n} {what}')
    from quanonet_amd.noise import DeviceNoise
    ideal, _ = _call(m, ins, y, DeviceNoise())
    assert np.abs(grad - ideal).max() > 1e-4                             # the setting shows in the buffer


@pytest.mark.parametrize('n', [7, 8, 9])
def test_uniform_setting_is_the_uniform_call(dev, n):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise, NoiseModel
    nm = NoiseModel(p1=0.03, p2=0.08, readout=0.04)
    kind, readout = ('quanonet', 'Y') if n != 8 else ('heaqnn', 'diag')
    m = _model(kind, n, True, readout, seed=n).to(dev)
    rows = 5
    ins, y = _inputs(kind, rows, dev, seed=5), _targets(rows, dev, 5)
    grad, pred = _call(m, ins, y, DeviceNoise.uniform(nm))
    flat = H.flat(m)
    want = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=dev)
    wpred = torch.zeros(rows, dtype=torch.float64, device=dev)
    _lib.model_loss_grad_noisy_exact_wide(m.fused_desc(), ins[0], _trunk(ins), y, flat, nm.params(), 1.0 / rows, want,
                                          ham_diag=_diag(m), pred=wpred)
    torch.cuda.synchronize()
    print(f'n={n} {kind}: {np.abs(grad - want.cpu().numpy()).max():.2e} {np.abs(pred - wpred.cpu().numpy()).max():.2e}')
    np.testing.assert_allclose(grad, want.cpu().numpy(), rtol=0, atol=ATOL)
    np.testing.assert_allclose(pred, wpred.cpu().numpy(), rtol=0, atol=ATOL)


@pytest.mark.parametrize('n', [7, 8, 9])
def test_default_setting_is_the_ideal_call(dev, n):
    """the check at a batch no numpy walk reaches: under DeviceNoise() the buffer is the ideal call's"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    kind, readout = ('heaqnn', 'diag') if n == 7 else ('quanonet', {8: 'X', 9: 'Z'}[n])
    m = _model(kind, n, True, readout, seed=n).to(dev)
    flat = H.flat(m)
    for rows in (1, 70):
        ins, y = _inputs(kind, rows, dev, seed=rows), _targets(rows, dev, rows)
        grad, pred = _call(m, ins, y, DeviceNoise())
        ideal = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=dev)
        ipred = torch.zeros(rows, dtype=torch.float64, device=dev)
        _lib.model_loss_grad(m.fused_desc(), ins[0], _trunk(ins), y, flat, 1.0 / rows, ideal, ham_diag=_diag(m), pred=ipred)
        torch.cuda.synchronize()
        np.testing.assert_allclose(grad, ideal.cpu().numpy(), rtol=0, atol=ATOL, err_msg=f'n={n} rows={rows}')
        np.testing.assert_allclose(pred, ipred.cpu().numpy(), rtol=0, atol=ATOL, err_msg=f'n={n} rows={rows}')


@pytest.mark.parametrize('n,kind,readout,rows,cuts', [(7, 'quanonet', 'Y', 37, (13,)), (8, 'heaqnn', 'Z', 11, (1, 4))])
def test_pred_bitwise_and_shards(dev, n, kind, readout, rows, cuts):
    from quanonet_amd import _lib
    m = _model(kind, n, True, readout, seed=3).to(dev)
    ins, y = _inputs(kind, rows, dev, seed=4), _targets(rows, dev, 4)
    dn = device_noise(n, True, seed=2)
    grad, pred = _call(m, ins, y, dn)
    # pred is the tiled device forward's, bit for bit
    fwd, _ = _lib.model_forward_noisy_device_exact_wide(m.fused_desc(), ins[0], _trunk(ins), H.flat(m), dn.params(n),
                                                        ham_diag=_diag(m))
    torch.cuda.synchronize()
    assert np.array_equal(pred, fwd.cpu().numpy())
    # two calls, with and without pred: bitwise
    grad2, pred2 = _call(m, ins, y, dn)
    grad3, _ = _call(m, ins, y, dn, want_pred=False)
    assert np.array_equal(grad, grad2) and np.array_equal(pred, pred2) and np.array_equal(grad, grad3)
    # shards of uneven size with the global inv_batch_total: a row's pred is bitwise the same at another batch, the buffers add
    # up to the whole call's; and a one-row call (whose buffer is that row's records, weighted) is bitwise reproducible
    bounds = (0,) + tuple(cuts) + (rows,)
    total, preds = 0.0, []
    for a, b in zip(bounds[:-1], bounds[1:]):
        g, p = _call(m, tuple(t[a:b] for t in ins), y[a:b], dn, inv=1.0 / rows)
        total = total + g
        preds.append(p)
    assert np.array_equal(np.concatenate(preds), pred)
    np.testing.assert_allclose(total, grad, rtol=0, atol=1e-12)
    one_a, pa = _call(m, tuple(t[:1] for t in ins), y[:1], dn, inv=1.0 / rows)
    one_b, pb = _call(m, tuple(t[:1].clone() for t in ins), y[:1].clone(), dn, inv=1.0 / rows)
    assert np.array_equal(one_a, one_b) and np.array_equal(pa, pred[:1]) and np.array_equal(pa, pb)


@pytest.mark.parametrize('n,kind,readout,trainable', [(7, 'quanonet', 'X', True), (8, 'heaqnn', 'diag', False)])
def test_train_steps(dev, n, kind, readout, trainable):
    """three steps with uneven bounds = the Python loop of loss_grad + adam_step, bitwise in parameters, moments and rows"""
    from quanonet_amd import _lib
    m = _model(kind, n, trainable, readout, seed=5).to(dev)
    bounds, sizes = [0, 5, 7, 14], [5, 2, 7]
    rows = bounds[-1]
    ins, y = _inputs(kind, rows, dev, seed=6), _targets(rows, dev, 6)
    desc, diag, trunk = m.fused_desc(), _diag(m), _trunk(ins)
    dn = device_noise(n, True, seed=3)
    lr, b1, b2, eps, wd = 3e-2, 0.9, 0.999, 1e-8, 0.0
    P = H.flat(m).numel()
    p1, m1, v1 = _adam_state(H.flat(m))
    out1 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
    _lib.model_train_steps_noisy_device_exact_wide(desc, bounds, sizes, ins[0], trunk, y, p1, out1, m1, v1, 1, lr, b1, b2, eps, wd,
                                                   dn.params(n), ham_diag=diag)
    p2, m2, v2 = _adam_state(H.flat(m))
    out2 = torch.zeros(3, P + 2, dtype=torch.float64, device=dev)
    for i in range(3):
        a, b = bounds[i], bounds[i + 1]
        _lib.model_loss_grad_noisy_device_exact_wide(desc, ins[0][a:b], None if trunk is None else trunk[a:b], y[a:b], p2,
                                                     dn.params(n), 1.0 / sizes[i], out2[i], ham_diag=diag)
        _lib.adam_step(p2, out2[i], m2, v2, i + 1, lr, b1, b2, eps, wd)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    assert not torch.equal(p1, H.flat(m)) and torch.all(torch.isfinite(out1))


def test_errors_launch_nothing(dev):
    """outputs prefilled with NaN stay NaN: a refused guard, a bad setting, a qubit count outside the range, a short workspace
    and a batch past the grid limit"""
    import ctypes
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    n = 7
    m = _model('quanonet', n, True, 'Z').to(dev)
    y = _targets(10, dev)
    nan = float('nan')

    def both(mod, kind, exc, rec):
        d, i, ref = mod.fused_desc(), _inputs(kind, 10, dev), H.flat(mod)
        Pm = ref.numel()
        full = lambda *shape: torch.full(shape, nan, dtype=torch.float64, device=dev)
        g, pr, mm, vv, out = full(Pm + 2), full(10), full(Pm), full(Pm), full(2, Pm + 2)
        p = ref.clone()
        with pytest.raises(exc):
            _lib.model_loss_grad_noisy_device_exact_wide(d, i[0], _trunk(i), y, p, rec, 0.1, g, pred=pr)
        with pytest.raises(exc):
            _lib.model_train_steps_noisy_device_exact_wide(d, [0, 4, 10], [4, 6], i[0], _trunk(i), y, p, out, mm, vv, 1, 1e-2, 0.9,
                                                           0.999, 1e-8, 0.0, rec)
        torch.cuda.synchronize()
        assert all(bool(torch.all(torch.isnan(t))) for t in (g, pr, mm, vv, out)) and torch.equal(p, ref)

    ok = dict(p1=0.01, p2=0.02, t1=1.0, t2=1.5, t_rx=0.01, t_rot=0.02, t_cx=0.03)
    # the guard: singular channels, and a decay whose amplification over this circuit passes 10^7
    for over in (dict(p1=0.75), dict(p2=15 / 16), dict(t_cx=1e4), dict(t_cx=2.0)):
        rec = DeviceNoise(**dict(ok, **over)).params(n)
        assert not _lib.model_device_noisy_log10_amplification(m.fused_desc(), rec) <= 7.0
        assert _lib.model_device_noisy_wide_refused(m.fused_desc(), rec)
        both(m, 'quanonet', _lib.Unsupported, rec)
    assert not _lib.model_device_noisy_wide_refused(m.fused_desc(), DeviceNoise(**ok).params(n))
    both(m, 'quanonet', _lib.QheaError, DeviceNoise(**ok).params(n - 1))          # a setting for another number of wires
    for nn in (6, 10):                                                            # the qubit counts on either side of the range
        mo = _model('heaqnn', nn, True, 'Z').to(dev)
        both(mo, 'heaqnn', _lib.Unsupported, DeviceNoise(**ok).params(nn))
    # a short workspace and a batch past the grid limit, through the C entry itself
    lib = _lib.load()
    d, ins, flat = m.fused_desc(), _inputs('quanonet', 10, dev), H.flat(m)
    rec = DeviceNoise(**ok).params(n)
    g = torch.full((flat.numel() + 2,), nan, dtype=torch.float64, device=dev)
    pr = torch.full((10,), nan, dtype=torch.float64, device=dev)
    need = _lib.model_device_noisy_wide_grad_workspace_bytes(d, 10)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ptr = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), ctypes.POINTER(ctypes.c_double))
    call = lambda batch, nbytes: lib.qhea_model_loss_grad_noisy_device_exact_wide(
        ctypes.byref(d), batch, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(flat), None, ctypes.byref(rec), 0.1, ptr(g), ptr(pr),
        ctypes.c_void_p(ws.data_ptr()), nbytes, None)
    assert call(10, need - 1) == -3
    assert call((2 ** 31 - 1 >> 2) + 1, 2 ** 62) == -1
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isnan(g))) and bool(torch.all(torch.isnan(pr))) and bool(torch.all(ws == 0))
    assert call(10, need) == 0                                                    # the same call with its workspace runs
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isfinite(g))) and bool(torch.all(torch.isfinite(pr)))


@pytest.mark.parametrize('n', [7, 9])
def test_graph_capturable_launch_count(dev, n):
    """one loss_grad call under capture: 6 + 4 (S + Z + R) launches plus the table kernel, one linear chain; the capture writes
    nothing; two replays are bitwise the eager result"""
    from quanonet_amd import _lib
    m = _model('quanonet', n, True, 'X').to(dev)                          # S = 2 sub-layers, Z = 2 empty blocks, R = 1
    S, Z, R = 2, 2, 1
    rows = 3
    ins, y = _inputs('quanonet', rows, dev), _targets(rows, dev)
    desc, flat = m.fused_desc(), H.flat(m)
    rec = device_noise(n, True, seed=4).params(n)
    P = flat.numel()

    def run(st):
        _lib.model_loss_grad_noisy_device_exact_wide(desc, ins[0], ins[1], y, flat, rec, 1.0 / rows, st[0], pred=st[1])

    fresh = lambda: (torch.full((P + 2,), float('nan'), dtype=torch.float64, device=dev),
                     torch.full((rows,), float('nan'), dtype=torch.float64, device=dev))
    eager = fresh()
    run(eager)                                                            # also sizes the workspace outside the capture
    torch.cuda.synchronize()
    assert all(bool(torch.all(torch.isfinite(t))) for t in eager)
    scratch = fresh()
    launches = H.kernel_launches(dev, lambda: run(scratch))
    names = [k[0] for k in launches]
    assert len(names) == 1 + 6 + 4 * (S + Z + R), names
    assert 'dev_wide_table_kernel' in names[0] and 'prep_model_kernel' in names[1], names
    assert _is_kernel(names[2], 'density_dev_wide_values_kernel', n), names
    fwd = names[3:3 + 2 * (S + Z + R)]
    assert sum(_is_kernel(k, 'density_dev_wide_ring_kernel', n) for k in fwd) == 2 * S
    assert sum(_is_kernel(k, 'density_dev_wide_wires_kernel', n) for k in fwd) == 2 * (Z + R)
    k0 = 3 + 2 * (S + Z + R)
    assert _is_kernel(names[k0], 'density_wide_readout_kernel', n) and _is_kernel(names[k0 + 1], 'density_wide_observable_kernel', n)
    back = names[k0 + 2:-2]
    assert sum(_is_kernel(k, 'density_dev_wide_ring_back_kernel', n) for k in back) == 2 * S
    assert sum(_is_kernel(k, 'density_dev_wide_enc_back_kernel', n) for k in back) == 2 * Z
    assert sum(_is_kernel(k, 'density_wide_wires_back_kernel', n) for k in back) == 2 * R
    assert len(back) == 2 * (S + Z + R)
    assert 'density_wide_fold_kernel' in names[-2] and 'reduce_density_kernel' in names[-1], names
    for k in launches:                                                    # every stage: one workgroup of 256 per (row, tile)
        if any(_is_kernel(k[0], ident, n) for ident in ('density_dev_wide_ring_kernel', 'density_dev_wide_wires_kernel',
                                                        'density_dev_wide_ring_back_kernel', 'density_dev_wide_enc_back_kernel',
                                                        'density_wide_wires_back_kernel', 'density_wide_observable_kernel')):
            assert k[1] == (rows * 4 ** (n - 6), 1, 1) and k[2] == (256, 1, 1), k
    st = fresh()
    s = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run(st)
    torch.cuda.synchronize()
    assert all(bool(torch.all(torch.isnan(t))) for t in st)               # the capture wrote nothing
    for _ in range(2):
        for t in st:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(st, eager):
            assert torch.equal(a, b)


def test_python_api(dev):
    from quanonet_amd.noise import NoiseModel, device_exact_noisy_loss_and_grad, device_noisy_loss_and_grad
    m5 = _model('quanonet', 5, True, 'X', seed=2).to(dev)
    ins, y = _inputs('quanonet', 37, dev, seed=2), _targets(37, dev, 2)
    dn5 = device_noise(5, True)
    a = device_exact_noisy_loss_and_grad(m5, ins, y.reshape(-1, 1), dn5)
    b = device_noisy_loss_and_grad(m5, ins, y.reshape(-1, 1), dn5)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    m7 = _model('heaqnn', 7, True, 'Y', seed=2).to(dev)
    ins7, y7 = _inputs('heaqnn', 3, dev, seed=2), _targets(3, dev, 2)
    dn7 = device_noise(7, False)
    got = device_exact_noisy_loss_and_grad(m7, ins7, y7.reshape(-1, 1), dn7)
    torch.cuda.synchronize()
    want, _ = _call(m7, ins7, y7, dn7)
    assert np.array_equal(got.cpu().numpy(), want)
    shard = device_exact_noisy_loss_and_grad(m7, ins7, y7, dn7, inv_batch_total=0.5)
    np.testing.assert_allclose(shard.cpu().numpy()[:-2], 1.5 * want[:-2], rtol=0, atol=ATOL)
    empty = device_exact_noisy_loss_and_grad(m7, tuple(t[:0] for t in ins7), y7[:0], dn7)
    assert empty.abs().sum().item() == 0.0
    with pytest.raises(ValueError, match='wide_exact_noisy_loss_and_grad'):
        device_exact_noisy_loss_and_grad(m7, ins7, y7, NoiseModel(p1=0.01))
    with pytest.raises(ValueError, match='n = 2..9'):
        device_exact_noisy_loss_and_grad(_model('heaqnn', 10, True, 'Z').to(dev), _inputs('heaqnn', 3, dev), y7, device_noise(10, True))


def _cfg(tmp_path, name, n=7, **kw):
    cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': n, 'net_size': [1, 1, 1, 0], 'scale_coeff': 0.5,
           'if_trainable_freq': 'true', 'learning_rate': 2e-2, 'batch_size': 10, 'num_epochs': 3, 'seed': 0,
           'prefix': str(tmp_path / name), 'run_id': 'r0', 'eval_batch_size': 64, 'trace_steps': True, 'if_save': False}
    cfg.update(kw)
    return cfg


def _data():
    return _solver_data(rows_train=40, rows_test=20)


def _run(tmp_path, name, dev, **kw):
    from quanonet_amd.solver import PTSolver, set_random_seed
    set_random_seed(0)
    lines = []
    s = PTSolver(_cfg(tmp_path, name, **kw), _data(), device=dev, log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return s, s.train(), lines


def _solver_noise(n):
    return device_noise(n, True, seed=5, scale=0.5)


def test_ptsolver_trains_and_resumes(dev, tmp_path):
    """three epochs of four batches at n = 7 with train_device_noise_exact='wide': the first step's loss is the helper's on the
    traced rows, the per-step path is the same run, a trainer that takes over parameters, moments and the Adam count after
    epoch 1 reproduces epochs 2 and 3 bitwise, and evaluate_noisy(dn, exact='device') scores the result"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import device_exact_noisy_predict
    from quanonet_amd.solver import regression_metrics
    n = 7
    dn = _solver_noise(n)
    keys = dict(train_device_noise=dn.asdict(), train_device_noise_exact='wide')
    s, hist, lines = _run(tmp_path, 'a', dev, **keys)
    t = s.trainer
    assert t.train_device_noise == dn and t.train_device_noise_exact == 'wide' and t.peer_fused is False
    said = [ln for ln in lines if 'device-noise training' in ln]
    desc = s.model.fused_desc()
    mib = _lib.model_device_noisy_wide_grad_workspace_bytes(desc, 10) / 2 ** 20
    amp = _lib.model_device_noisy_log10_amplification(desc, dn.params(n))
    assert len(said) == 1 and 'exact device-noisy MSE' in said[0] and f'log10 A_dev {amp:.2f}' in said[0] \
        and f'{mib:.1f} MiB for steps of up to 10 rows' in said[0], said
    nb = len(hist['loss_steps']) // 3
    assert len(hist['loss_train']) == 3 and nb == 4 and all(np.isfinite(hist['loss_steps']))
    assert hist['loss_train'][-1] < hist['loss_train'][0]
    # the first step's loss: the helper on the traced rows with the initial parameters
    data = _data()
    idx = np.asarray(hist['indices'][0])[:10]
    init = _run(tmp_path, 'init', dev, num_epochs=0, **keys)[0].model
    ref, _ = DV.model_loss_grad(DG.spec_of(init), H.flat(init).cpu().numpy(), data['train_branch_input'][idx],
                                data['train_trunk_input'][idx], data['train_output'][idx, 0], as_dict(dn, n), 1.0 / 10, inverse=True)
    print(f"first step: loss {hist['loss_steps'][0]:.12f}, helper {ref[-2] / 10:.12f}")
    assert abs(hist['loss_steps'][0] - ref[-2] / 10) < ATOL
    _, ideal, _ = _run(tmp_path, 'ideal', dev)
    assert ideal['loss_steps'][0] != hist['loss_steps'][0]
    _, per_step, _ = _run(tmp_path, 'steps', dev, epoch_call=False, **keys)
    assert per_step['loss_steps'] == hist['loss_steps']
    # resumed after epoch 1
    s1, h1, _ = _run(tmp_path, 'one', dev, num_epochs=1, **keys)
    assert h1['loss_steps'] == hist['loss_steps'][:nb]
    s2 = _run(tmp_path, 'rest', dev, num_epochs=0, **keys)[0]
    t1, t2 = s1.trainer, s2.trainer
    t2.pflat.copy_(t1.pflat)
    t2.optimizer.exp_avg.copy_(t1.optimizer.exp_avg)
    t2.optimizer.exp_avg_sq.copy_(t1.optimizer.exp_avg_sq)
    t2.optimizer.t = t1.optimizer.t
    tens = lambda k, i: torch.tensor(np.asarray(data[k], np.float64)[i], device=dev)
    losses = []
    for ep in (1, 2):
        order = np.asarray(hist['indices'][ep])
        for a in range(0, len(order), 10):
            i = order[a:a + 10]
            flat = t2.train_step(tens('train_branch_input', i), tens('train_trunk_input', i), tens('train_output', i)[:, 0],
                                 global_batch=len(i))
            losses.append(float(flat[-2]) / len(i))
    torch.cuda.synchronize()
    assert torch.equal(t2.pflat, t.pflat)
    assert losses == hist['loss_steps'][nb:]
    # scored on the loss it was trained on
    res = s.evaluate_noisy(dn, exact='device')
    pred, _ = device_exact_noisy_predict(s.model, s.test_input, dn)
    assert res['MSE'] == regression_metrics(pred, torch.tensor(data['test_output'], device=dev))['MSE']


def test_ptsolver_small_n_is_train_device_noise_alone(dev, tmp_path):
    """n = 2: the key changes nothing -- the run that train_device_noise alone describes, bitwise, stored states included"""
    dn = device_noise(2, True, seed=5).asdict()
    for states in (None, 'stored'):
        runs = []
        for name, kw in (('alone', {}), ('wide', dict(train_device_noise_exact='wide'))):
            s, hist, _ = _run(tmp_path, f'{name}_{states}', dev, n=2, net_size=[2, 1, 2, 1], train_device_noise=dn,
                              train_noise_states=states, **kw)
            runs.append((hist['loss_steps'], H.flat(s.model).clone()))
        assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


def test_refusals(dev, tmp_path):
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import NoiseModel, Sampling
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    from quanonet_amd.solver import DataParallelTrainer, PTSolver
    from quanonet_amd.sweep import SweepSolver
    data = _data()
    quiet = lambda *a, **k: None
    dn = _solver_noise(7)
    solver = lambda name, **kw: PTSolver(_cfg(tmp_path, name, **kw), data, device=dev, log=quiet)
    with pytest.raises(ValueError, match="None or 'wide'"):
        solver('value', train_device_noise=dn, train_device_noise_exact='tiled')
    with pytest.raises(ValueError, match='needs train_device_noise'):
        solver('alone', train_device_noise_exact='wide')
    with pytest.raises(ValueError, match='train_noise'):
        solver('uniform', train_noise=NoiseModel(p1=0.01), train_device_noise_exact='wide')
    sp = Sampling(trajectories=8, seed=1)
    for key in ('train_sampling', 'train_trajectories', 'train_jump_trajectories'):
        with pytest.raises(ValueError, match=key):
            solver(key, train_device_noise=dn, train_device_noise_exact='wide', **{key: sp})
    with pytest.raises(ValueError, match='does not exist on tiles'):
        solver('states', train_device_noise=dn, train_device_noise_exact='wide', train_noise_states='stored')
    with pytest.raises(ValueError, match='n <= 9'):
        solver('n10', n=10, train_device_noise=_solver_noise(10), train_device_noise_exact='wide')
    with pytest.raises(ValueError, match=r'A_dev = .*bound is 7'):          # past the guard: A_dev and the bound are named
        solver('guard', train_device_noise=device_noise(7, True, scale=8.0), train_device_noise_exact='wide')
    with pytest.raises(ValueError, match='A_dev = inf'):                    # a singular channel
        solver('singular', train_device_noise=dict(dn.asdict(), p1=[0.75] * 7), train_device_noise_exact='wide')
    # the existing key beside a DeviceNoise still raises, and train_device_noise alone at n = 7 raises as before
    with pytest.raises(ValueError, match='train_device_noise'):
        solver('other', train_device_noise=dn, train_noise_exact='wide')
    with pytest.raises(ValueError, match='n <= 6'):
        solver('plain7', train_device_noise=dn)
    # a non-fused model or optimizer
    m = _model('quanonet', 7, True, 'Z').to(dev)
    with pytest.raises(ValueError, match='fused'):
        DataParallelTrainer(m, fused=False, train_device_noise=dn, train_device_noise_exact='wide')
    with pytest.raises(ValueError, match='fused'):
        DataParallelTrainer(m, optimizer='sgd', train_device_noise=dn, train_device_noise_exact='wide')
    # the four member solvers
    for cls in (EnsembleSolver, SweepSolver, DepthSweepSolver, QubitSweepSolver):
        cfgs = [_cfg(tmp_path, cls.__name__, n=2, net_size=[2, 1, 2, 1], seed=k, run_id=f'm{k}') for k in (0, 1)]
        cfgs[1]['train_device_noise_exact'] = 'wide'
        with pytest.raises(ValueError, match='train_device_noise_exact'):
            cls(cfgs, data, device=dev, log=quiet)
