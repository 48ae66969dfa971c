"""
Exact device-noise training from stored states at n = 7..9 on the GPU (qhea_model_loss_grad_noisy_device_exact_wide_stored /
qhea_model_train_steps_noisy_device_exact_wide_stored, device_exact_noisy_loss_and_grad(states='stored'), PTSolver with
train_device_noise_exact='stored') against the stored walk of the numpy helper tests/device_noise_grad_reference.py
(model_loss_grad(..., inverse=False)): past the inverse walk's bound, where that call refuses and the helper's two walks differ
by more than ten times the tolerance (tests/test_device_exact_noisy_wide_stored_training_abi.py asserts that on the CPU, on the
same inputs); inside the bound beside the inverse call, pred bitwise that call's and the tiled device forward's; a snapshot
region past 4 GiB; reproducibility, shards and train_steps = the loop of single calls; refusals with untouched outputs; the
launch count of the header under graph capture; the Python surface.  Tolerance against the helper: atol 1e-10, as everywhere.
The shapes are those of tests/test_device_exact_noisy_wide_training.py: blocks of depth 0 (encoding-only units of both stages), 1
and 2 (ring units with and without the encoding), 1..3 rows; the helper's walk takes seconds per row at n = 9, so n = 8, 9 use
one row.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import density_grad_reference as DG
from tests import device_noise_grad_reference as DV
from tests import helpers as H
from tests.test_device_exact_noisy_wide import _net_model
from tests.test_device_exact_noisy_wide_stored_training_abi import PAST_NET, PAST_THE_BOUND
from tests.test_device_exact_noisy_wide_training import _cfg, _data, _edge_setting, _run
from tests.test_device_noise_stored_training import past_the_bound_case, past_the_bound_model
from tests.test_device_noise_training_abi import MAX_LOG10_AMPLIFICATION, as_dict, device_noise, probe_setting
from tests.test_exact_noisy_wide_training import _adam_state, _diag, _is_kernel, _model, _targets
from tests.test_noisy_forward import _inputs

pytestmark = pytest.mark.gpu
ATOL = 1e-10


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _trunk(ins):
    return ins[1] if len(ins) > 1 else None


def _call(m, ins, y, dn, inv=None, want_pred=True, flat=None, states='stored'):
    """(grad[P+2], pred[B]) of one loss_grad call (the stored-state one, or with states='inverse' the inverse walk's) as numpy
    arrays"""
    from quanonet_amd import _lib
    flat = H.flat(m) if flat is None else flat
    rows = ins[0].shape[0]
    grad = torch.full((flat.numel() + 2,), -77.0, dtype=torch.float64, device=flat.device)
    pred = torch.full((rows,), -77.0, dtype=torch.float64, device=flat.device) if want_pred else None
    call = _lib.model_loss_grad_noisy_device_exact_wide_stored if states == 'stored' else _lib.model_loss_grad_noisy_device_exact_wide
    call(m.fused_desc(), ins[0], _trunk(ins), y, flat, dn.params(m.num_qubits), 1.0 / rows if inv is None else inv, grad,
         ham_diag=_diag(m), pred=pred)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (pred.cpu().numpy() if want_pred else None)


def _helper(m, ins, y, dn):
    """the helper's stored walk: ([P + 2], pred)"""
    rows = ins[0].shape[0]
    return DV.model_loss_grad(DG.spec_of(m), H.flat(m).cpu().numpy(), ins[0].cpu().numpy(),
                              ins[1].cpu().numpy() if len(ins) > 1 else None, y.cpu().numpy(), as_dict(dn, m.num_qubits),
                              1.0 / rows, inverse=False)


def _forward(m, ins, dn):
    from quanonet_amd import _lib
    fwd, _ = _lib.model_forward_noisy_device_exact_wide(m.fused_desc(), ins[0], _trunk(ins), H.flat(m), dn.params(m.num_qubits),
                                                        ham_diag=_diag(m))
    torch.cuda.synchronize()
    return fwd.cpu().numpy()


@pytest.mark.parametrize('n,target', PAST_THE_BOUND)
def test_past_the_bound(dev, n, target):
    """log10 A_dev = 16 and 20 on a fixed-frequency HEAQNN (3, 2) with angles all over the circle, one row: the inverse call
    refuses, the layer value is within the bound, the stored call matches the helper's stored walk, and the gradient is not a
    vanishing one.  On these inputs the helper's inverse walk is further than 1e-9 from its stored walk (asserted on the CPU in
    test_device_exact_noisy_wide_stored_training_abi.py), so a kernel that walked rho back would fail here."""
    from quanonet_amd import _lib
    from quanonet_amd.noise import device_amplification, device_layer_amplification
    spec, flat, x, y, dn, logA = past_the_bound_case(n, PAST_NET, target, 1)
    m = past_the_bound_model(n, PAST_NET)
    layer = device_layer_amplification(m, dn)
    assert abs(device_amplification(m, dn) - target) < 1e-6 and layer <= MAX_LOG10_AMPLIFICATION
    m, ins, y = m.to(dev), (torch.tensor(x, device=dev),), torch.tensor(y, device=dev)
    with pytest.raises(_lib.Unsupported):
        _call(m, ins, y, dn, states='inverse')
    grad, pred = _call(m, ins, y, dn)
    ref, ref_pred = _helper(m, ins, y, dn)
    print(f'n={n} net={PAST_NET} log10 A_dev={logA:.2f} (layer {layer:.2f}): max|grad - helper|={np.abs(grad - ref).max():.2e} '
          f'max|pred - helper|={np.abs(pred - ref_pred).max():.2e} max|gradient|={np.abs(grad[:-2]).max():.2e}')
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL)
    assert np.abs(grad[:-2]).max() >= 1e-3


def _inside(m, ins, y, dn, tag):
    """inside the bound: the helper's stored walk and the inverse call within 1e-10, pred bitwise the inverse call's and the tiled
    device forward's"""
    grad, pred = _call(m, ins, y, dn)
    ref, ref_pred = _helper(m, ins, y, dn)
    inv, inv_pred = _call(m, ins, y, dn, states='inverse')
    print(f'{tag}: max|grad - helper|={np.abs(grad - ref).max():.2e} max|pred - helper|={np.abs(pred - ref_pred).max():.2e} '
          f'max|grad - inverse call|={np.abs(grad - inv).max():.2e} max|grad|={np.abs(ref[:-2]).max():.2e}')
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=0, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(grad, inv, rtol=0, atol=ATOL, err_msg=tag)
    assert np.array_equal(pred, inv_pred), tag
    assert np.array_equal(pred, _forward(m, ins, dn)), tag
    return grad


# 'quanonet' (net (2, 0, 1, 2)): a block of two sub-layers and two without; 'heaqnn' (net (3, 1)): three blocks of one sub-layer
@pytest.mark.parametrize('readout', ['Z', 'X', 'Y', 'diag'])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_inside_the_bound_n7(dev, kind, readout):
    n = 7
    m = _model(kind, n, True, readout, seed=n).to(dev)
    for rows, idle in ((1, True), (1, False), (3, True), (3, False)):
        ins, y = _inputs(kind, rows, dev, seed=rows), _targets(rows, dev, rows)
        _inside(m, ins, y, device_noise(n, idle, seed=rows), f'n={n} {kind} {readout} rows={rows} idle={idle}')


@pytest.mark.parametrize('n,readout,idle', [(8, 'diag', True), (9, 'X', False)])
def test_inside_the_bound_n8_n9(dev, n, readout, idle):
    """one row on the blocks (n, 1), (n, 0): a QuanONet of net (1, 0, 1, 1)"""
    from oracle import hea_oracle as O
    assert O.block_configs_quanonet(n, (1, 0, 1, 1)) == [(n, 1), (n, 0)]
    m = _net_model('quanonet', n, (1, 0, 1, 1), readout, seed=n).to(dev)
    ins, y = _inputs('quanonet', 1, dev, seed=n), _targets(1, dev, n)
    _inside(m, ins, y, device_noise(n, idle, seed=1), f'n={n} quanonet {readout} idle={idle}')


@pytest.mark.parametrize('what', ['closing-pair', 'wire-6', 'readout-top-bit', 'p2-closing-slot'])
@pytest.mark.parametrize('n', [7, 9])
def test_device_site_edges(dev, n, what):
    """where the device sites can go wrong, each alone, on blocks (n, 1), (n, 0), one row"""
    from quanonet_amd.noise import DeviceNoise
    m = _net_model('quanonet', n, (1, 0, 1, 1), 'Y' if what != 'readout-top-bit' else 'Z', seed=n + 2).to(dev)
    ins, y = _inputs('quanonet', 1, dev, seed=n + 1), _targets(1, dev, n + 1)
    grad = _inside(m, ins, y, _edge_setting(what, n), f'n={n} {what}')
    ideal, _ = _call(m, ins, y, DeviceNoise())
    assert np.abs(grad - ideal).max() > 1e-4                             # the setting shows in the buffer


def test_snapshots_past_4_gib(dev):
    """n = 9, HEAQNN (3, 2): 6 units of 4 MiB per row, so 180 rows are 4.2 GiB of snapshots and the last units' offsets do not fit
    32 bits.  Under DeviceNoise() the buffer is the ideal call's; under a per-wire setting with idle decay the inverse call's.
    That setting is device_noise(9, True, scale=0.5), log10 A_dev 5.15: at scale 1 this shape has log10 A_dev 10.36 and the
    inverse call, the reference here, refuses it (asserted) -- there the 180 rows' pred is held to the tiled device forward's
    bit for bit, and a one-row call before and after the large ones is bitwise the same (the snapshot region moves with the
    batch) and is row 0 of the large call."""
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise, device_amplification
    n, rows = 9, 180
    m = H.heaqnn(n, 4, (3, 2), 1, if_trainable_freq=True, scale_coeff=0.7, ham_bound=(-2.0, 3.0)).to(dev)
    desc = m.fused_desc()
    snap = _lib.model_device_noisy_wide_stored_grad_workspace_bytes(desc, rows, snapshots_only=True)
    assert snap == 6 * rows * 16 * 4 ** n and snap > 1 << 32
    rng = np.random.default_rng(9)
    ins = (torch.tensor(rng.uniform(-1, 1, (rows, 4)), device=dev),)
    y = torch.tensor(rng.normal(scale=0.7, size=rows), device=dev)
    past, dn = device_noise(n, True), device_noise(n, True, scale=0.5)
    assert device_amplification(m, past) > MAX_LOG10_AMPLIFICATION > device_amplification(m, dn) > 5.0
    one = tuple(t[:1] for t in ins)
    first, first_pred = _call(m, one, y[:1], past, inv=1.0 / rows)
    flat = H.flat(m)
    ideal = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=dev)
    ipred = torch.zeros(rows, dtype=torch.float64, device=dev)
    _lib.model_loss_grad(desc, ins[0], None, y, flat, 1.0 / rows, ideal, ham_diag=_diag(m), pred=ipred)
    torch.cuda.synchronize()
    grad0, pred0 = _call(m, ins, y, DeviceNoise())
    print(f'Q9, 6 units, {rows} rows, {snap} snapshot bytes, DeviceNoise(): max|grad - ideal call|='
          f'{np.abs(grad0 - ideal.cpu().numpy()).max():.2e} max|pred - ideal call|={np.abs(pred0 - ipred.cpu().numpy()).max():.2e}')
    np.testing.assert_allclose(grad0, ideal.cpu().numpy(), rtol=0, atol=ATOL)
    np.testing.assert_allclose(pred0, ipred.cpu().numpy(), rtol=0, atol=ATOL)
    grad, pred = _call(m, ins, y, dn)
    inv, inv_pred = _call(m, ins, y, dn, states='inverse')
    print(f'... device_noise(9, True, scale=0.5): max|grad - inverse call|={np.abs(grad - inv).max():.2e} '
          f'max|gradient|={np.abs(grad[:-2]).max():.2e}')
    np.testing.assert_allclose(grad, inv, rtol=0, atol=ATOL)
    assert np.array_equal(pred, inv_pred)
    assert np.abs(grad[:-2]).max() >= 1e-3
    with pytest.raises(_lib.Unsupported):
        _call(m, ins, y, past, states='inverse')
    grad1, pred1 = _call(m, ins, y, past)
    assert np.array_equal(pred1, _forward(m, ins, past)) and np.all(np.isfinite(grad1))
    again, again_pred = _call(m, one, y[:1], past, inv=1.0 / rows)
    assert np.array_equal(first, again) and np.array_equal(first_pred, again_pred) and np.array_equal(first_pred, pred1[:1])


def _past_the_bound_on(dev, rows, n=7, target=16.0, seed=0):
    """the model of test_past_the_bound at n with `rows` rows on the device, and its setting"""
    m = past_the_bound_model(n, PAST_NET)
    dn, _ = probe_setting(n, [(n, PAST_NET[1])] * PAST_NET[0], target)
    rng = np.random.default_rng(seed)
    ins = (torch.tensor(rng.uniform(-1, 1, (rows, 4)), device=dev),)
    return m.to(dev), ins, torch.tensor(rng.normal(scale=0.7, size=rows), device=dev), dn


@pytest.mark.parametrize('n,kind,readout,rows,cuts', [(7, 'quanonet', 'Y', 37, (13,)), (8, 'heaqnn', 'Z', 11, (1, 4))])
def test_bitwise_and_shards(dev, n, kind, readout, rows, cuts):
    m = _model(kind, n, True, readout, seed=3).to(dev)
    ins, y = _inputs(kind, rows, dev, seed=4), _targets(rows, dev, 4)
    dn = device_noise(n, True, seed=2)
    grad, pred = _call(m, ins, y, dn)
    assert np.array_equal(pred, _forward(m, ins, dn))
    # two calls, with and without pred: bitwise
    grad2, pred2 = _call(m, ins, y, dn)
    grad3, _ = _call(m, ins, y, dn, want_pred=False)
    assert np.array_equal(grad, grad2) and np.array_equal(pred, pred2) and np.array_equal(grad, grad3)
    # shards of uneven size with the global inv_batch_total
    bounds = (0,) + tuple(cuts) + (rows,)
    total, preds = 0.0, []
    for a, b in zip(bounds[:-1], bounds[1:]):
        g, p = _call(m, tuple(t[a:b] for t in ins), y[a:b], dn, inv=1.0 / rows)
        total = total + g
        preds.append(p)
    assert np.array_equal(np.concatenate(preds), pred)
    np.testing.assert_allclose(total, grad, rtol=0, atol=1e-12)


def test_train_steps_is_the_loop_of_single_calls(dev):
    """two steps of unequal batch past the bound (the workspace is sized by the larger, the snapshots lie behind its regions):
    bitwise the Python loop of loss_grad + adam_step in parameters, moments and rows"""
    from quanonet_amd import _lib
    n = 7
    bounds, sizes = [0, 2, 7], [2, 5]
    m, ins, y, dn = _past_the_bound_on(dev, bounds[-1])
    desc, rec, diag = m.fused_desc(), dn.params(n), _diag(m)
    assert _lib.model_device_noisy_wide_refused(desc, rec) and not _lib.model_device_noisy_wide_stored_refused(desc, rec)
    lr, b1, b2, eps, wd = 3e-2, 0.9, 0.999, 1e-8, 0.0
    P = H.flat(m).numel()
    p1, m1, v1 = _adam_state(H.flat(m))
    out1 = torch.zeros(2, P + 2, dtype=torch.float64, device=dev)
    _lib.model_train_steps_noisy_device_exact_wide_stored(desc, bounds, sizes, ins[0], None, y, p1, out1, m1, v1, 1, lr, b1, b2, eps,
                                                          wd, rec, ham_diag=diag)
    p2, m2, v2 = _adam_state(H.flat(m))
    out2 = torch.zeros(2, P + 2, dtype=torch.float64, device=dev)
    for i in range(2):
        a, b = bounds[i], bounds[i + 1]
        _lib.model_loss_grad_noisy_device_exact_wide_stored(desc, ins[0][a:b], None, y[a:b], p2, rec, 1.0 / sizes[i], out2[i],
                                                            ham_diag=diag)
        _lib.adam_step(p2, out2[i], m2, v2, i + 1, lr, b1, b2, eps, wd)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    assert not torch.equal(p1, H.flat(m)) and torch.all(torch.isfinite(out1))


def test_errors_launch_nothing(dev):
    """outputs prefilled with NaN stay NaN: the qubit counts on either side of the range, a layer amplification above the bound,
    a singular channel, a bad setting and a workspace one byte short"""
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
            _lib.model_loss_grad_noisy_device_exact_wide_stored(d, i[0], _trunk(i), y, p, rec, 0.1, g, pred=pr)
        with pytest.raises(exc):
            _lib.model_train_steps_noisy_device_exact_wide_stored(d, [0, 4, 10], [4, 6], i[0], _trunk(i), y, p, out, mm, vv, 1, 1e-2,
                                                                  0.9, 0.999, 1e-8, 0.0, rec)
        torch.cuda.synchronize()
        assert all(bool(torch.all(torch.isnan(t))) for t in (g, pr, mm, vv, out)) and torch.equal(p, ref)

    ok = dict(p1=0.01, p2=0.02, t1=1.0, t2=1.5, t_rx=0.01, t_rot=0.02, t_cx=0.03)
    desc = m.fused_desc()
    # a layer amplification above 7 without a singular channel (p2 = 0.9: 1.40 per slot), and singular channels
    rec = DeviceNoise(**dict(ok, p2=0.9)).params(n)
    layer = _lib.model_device_noisy_log10_layer_amplification(desc, rec)
    assert MAX_LOG10_AMPLIFICATION < layer < float('inf')
    assert _lib.model_device_noisy_wide_stored_refused(desc, rec)
    both(m, 'quanonet', _lib.Unsupported, rec)
    for over in (dict(p1=0.75), dict(p2=15 / 16), dict(t_cx=1e4)):
        rec = DeviceNoise(**dict(ok, **over)).params(n)
        assert _lib.model_device_noisy_log10_layer_amplification(desc, rec) == float('inf')
        assert _lib.model_device_noisy_wide_stored_refused(desc, rec)
        both(m, 'quanonet', _lib.Unsupported, rec)
    assert not _lib.model_device_noisy_wide_stored_refused(desc, DeviceNoise(**ok).params(n))
    both(m, 'quanonet', _lib.QheaError, DeviceNoise(**ok).params(n - 1))          # a setting for another number of wires
    for nn in (6, 10):                                                            # the qubit counts on either side of the range
        mo = _model('heaqnn', nn, True, 'Z').to(dev)
        both(mo, 'heaqnn', _lib.Unsupported, DeviceNoise(**ok).params(nn))
    # a workspace one byte short, through the C entry itself
    lib = _lib.load()
    ins, flat = _inputs('quanonet', 10, dev), H.flat(m)
    rec = DeviceNoise(**ok).params(n)
    g = torch.full((flat.numel() + 2,), nan, dtype=torch.float64, device=dev)
    pr = torch.full((10,), nan, dtype=torch.float64, device=dev)
    need = _lib.model_device_noisy_wide_stored_grad_workspace_bytes(desc, 10)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ptr = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), ctypes.POINTER(ctypes.c_double))
    call = lambda batch, nbytes: lib.qhea_model_loss_grad_noisy_device_exact_wide_stored(
        ctypes.byref(desc), batch, ptr(ins[0]), ptr(ins[1]), ptr(y), ptr(flat), None, ctypes.byref(rec), 0.1, ptr(g), ptr(pr),
        ctypes.c_void_p(ws.data_ptr()), nbytes, None)
    assert call(10, need - 1) == -3
    assert call(10, _lib.model_device_noisy_wide_grad_workspace_bytes(desc, 10)) == -3
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isnan(g))) and bool(torch.all(torch.isnan(pr))) and bool(torch.all(ws == 0))
    assert call(10, need) == 0                                                    # the same call with its workspace runs
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isfinite(g))) and bool(torch.all(torch.isfinite(pr)))


@pytest.mark.parametrize('n', [7, 9])
def test_graph_capturable_launch_count(dev, n):
    """one loss_grad call under capture: 6 + 4 (S + Z + R) launches plus the table kernel, as the inverse call, one linear chain;
    stage A of every forward unit and of the basis change is the source/destination form, every reverse stage the `from` form;
    two replays are bitwise the eager result"""
    from quanonet_amd import _lib
    m = _model('quanonet', n, True, 'X').to(dev)                          # S = 2 sub-layers, Z = 2 empty blocks, R = 1
    S, Z, R = 2, 2, 1
    rows = 3
    ins, y = _inputs('quanonet', rows, dev), _targets(rows, dev)
    desc, flat = m.fused_desc(), H.flat(m)
    rec = device_noise(n, True, seed=4).params(n)
    P = flat.numel()

    def run(st):
        _lib.model_loss_grad_noisy_device_exact_wide_stored(desc, ins[0], ins[1], y, flat, rec, 1.0 / rows, st[0], pred=st[1])

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
    assert sum(_is_kernel(k, 'density_dev_wide_ring_to_kernel', n) for k in fwd) == S
    assert sum(_is_kernel(k, 'density_dev_wide_ring_kernel', n) for k in fwd) == S
    assert sum(_is_kernel(k, 'density_dev_wide_wires_to_kernel', n) for k in fwd) == Z + R
    assert sum(_is_kernel(k, 'density_dev_wide_wires_kernel', n) for k in fwd) == Z + R
    k0 = 3 + 2 * (S + Z + R)
    assert _is_kernel(names[k0], 'density_wide_readout_kernel', n) and _is_kernel(names[k0 + 1], 'density_wide_observable_kernel', n)
    back = names[k0 + 2:-2]
    assert sum(_is_kernel(k, 'density_dev_wide_ring_back_from_kernel', n) for k in back) == 2 * S
    assert sum(_is_kernel(k, 'density_dev_wide_enc_back_from_kernel', n) for k in back) == 2 * Z
    assert sum(_is_kernel(k, 'density_wide_wires_back_kernel', n) for k in back) == 2 * R
    assert len(back) == 2 * (S + Z + R)
    assert 'density_wide_fold_kernel' in names[-2] and 'reduce_density_kernel' in names[-1], names
    for k in launches:                                                    # every stage: one workgroup of 256 per (row, tile)
        if any(_is_kernel(k[0], ident, n) for ident in ('density_dev_wide_ring_to_kernel', 'density_dev_wide_wires_to_kernel',
                                                        'density_dev_wide_ring_kernel', 'density_dev_wide_wires_kernel',
                                                        'density_dev_wide_ring_back_from_kernel',
                                                        'density_dev_wide_enc_back_from_kernel',
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
    from quanonet_amd.noise import device_exact_noisy_loss_and_grad, device_noisy_loss_and_grad
    m3 = _model('quanonet', 3, True, 'X', seed=2).to(dev)
    ins, y = _inputs('quanonet', 37, dev, seed=2), _targets(37, dev, 2)
    dn3 = device_noise(3, True)
    a = device_exact_noisy_loss_and_grad(m3, ins, y.reshape(-1, 1), dn3, states='stored')
    b = device_noisy_loss_and_grad(m3, ins, y.reshape(-1, 1), dn3, states='stored')
    c = device_exact_noisy_loss_and_grad(m3, ins, y.reshape(-1, 1), dn3)
    d = device_noisy_loss_and_grad(m3, ins, y.reshape(-1, 1), dn3)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(c, d)
    m7, ins7, y7, dn7 = _past_the_bound_on(dev, 2, seed=3)
    got = device_exact_noisy_loss_and_grad(m7, ins7, y7.reshape(-1, 1), dn7, states='stored')
    torch.cuda.synchronize()
    want, _ = _call(m7, ins7, y7, dn7)
    assert np.array_equal(got.cpu().numpy(), want)
    shard = device_exact_noisy_loss_and_grad(m7, ins7, y7, dn7, inv_batch_total=0.25, states='stored')
    np.testing.assert_allclose(shard.cpu().numpy()[:-2], 0.5 * want[:-2], rtol=0, atol=ATOL)
    empty = device_exact_noisy_loss_and_grad(m7, tuple(t[:0] for t in ins7), y7[:0], dn7, states='stored')
    assert empty.abs().sum().item() == 0.0
    from quanonet_amd import _lib
    with pytest.raises(_lib.Unsupported):                                # the default is the inverse walk, which refuses this setting
        device_exact_noisy_loss_and_grad(m7, ins7, y7, dn7)
    with pytest.raises(ValueError, match="'inverse' or 'stored'"):
        device_exact_noisy_loss_and_grad(m7, ins7, y7, dn7, states='snapshots')


PAST_SOLVER_NET = [2, 2, 1, 2]             # six sub-layers at n = 7: log10 A_dev 12.91 in total, 2.31 for one layer under _past_noise


def _past_noise(n=7):
    """a setting past the inverse walk's bound for a QuanONet of net PAST_SOLVER_NET and inside the layer bound"""
    return device_noise(n, True, seed=5, scale=2.0)


def test_ptsolver_trains_past_the_bound(dev, tmp_path):
    """two epochs of four batches at n = 7 with train_device_noise_exact='stored' under a setting 'wide' refuses: loss_steps are a
    hand loop of train_step bitwise, the log line names both amplifications, the snapshot bytes and the workspace, and
    evaluate_noisy(dn, exact='device') scores with the same forward"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import device_exact_noisy_predict
    from quanonet_amd.solver import regression_metrics
    n = 7
    dn = _past_noise(n)
    keys = dict(train_device_noise=dn.asdict(), train_device_noise_exact='stored', num_epochs=2, net_size=PAST_SOLVER_NET)
    with pytest.raises(ValueError, match=r'A_dev = .*bound is 7'):
        _run(tmp_path, 'wide', dev, **dict(keys, train_device_noise_exact='wide'))
    s, hist, lines = _run(tmp_path, 'a', dev, **keys)
    t = s.trainer
    assert t.train_device_noise == dn and t.train_device_noise_exact == 'stored' and t.noise_states == 'stored'
    assert t.peer_fused is False
    desc = s.model.fused_desc()
    rec = dn.params(n)
    amp = _lib.model_device_noisy_log10_amplification(desc, rec)
    layer = _lib.model_device_noisy_log10_layer_amplification(desc, rec)
    assert amp > MAX_LOG10_AMPLIFICATION >= layer
    per_row = _lib.model_device_noisy_wide_stored_grad_workspace_bytes(desc, 1, snapshots_only=True)
    mib = _lib.model_device_noisy_wide_stored_grad_workspace_bytes(desc, 10) / 2 ** 20
    said = [ln for ln in lines if 'device-noise training' in ln]
    assert len(said) == 1 and 'exact device-noisy MSE' in said[0] and 'stored states' in said[0] \
        and f'log10 A_dev {amp:.2f} in total' in said[0] and f'{layer:.2f} for one layer' in said[0] \
        and f'{per_row} snapshot bytes per row' in said[0] and f'{mib:.1f} MiB for steps of up to 10 rows' in said[0], said
    nb = len(hist['loss_steps']) // 2
    assert len(hist['loss_train']) == 2 and nb == 4 and all(np.isfinite(hist['loss_steps']))
    # the same run with train_noise_states='stored' beside the key, and step by step
    _, same, _ = _run(tmp_path, 'b', dev, train_noise_states='stored', **keys)
    assert same['loss_steps'] == hist['loss_steps']
    _, per_step, _ = _run(tmp_path, 'steps', dev, epoch_call=False, **keys)
    assert per_step['loss_steps'] == hist['loss_steps']
    # a hand loop of train_step on the traced rows
    data = _data()
    s2 = _run(tmp_path, 'hand', dev, **dict(keys, num_epochs=0))[0]
    t2 = s2.trainer
    tens = lambda k, i: torch.tensor(np.asarray(data[k], np.float64)[i], device=dev)
    losses = []
    for ep in (0, 1):
        order = np.asarray(hist['indices'][ep])
        for a in range(0, len(order), 10):
            i = order[a:a + 10]
            flat = t2.train_step(tens('train_branch_input', i), tens('train_trunk_input', i), tens('train_output', i)[:, 0],
                                 global_batch=len(i))
            losses.append(float(flat[-2]) / len(i))
    torch.cuda.synchronize()
    assert losses == hist['loss_steps'] and torch.equal(t2.pflat, t.pflat)
    # scored on the loss it was trained on
    res = s.evaluate_noisy(dn, exact='device')
    pred, _ = device_exact_noisy_predict(s.model, s.test_input, dn)
    assert res['MSE'] == regression_metrics(pred, torch.tensor(data['test_output'], device=dev))['MSE']


def test_ptsolver_small_n_is_train_noise_states_stored(dev, tmp_path):
    """n = 2: 'stored' is the run that train_device_noise with train_noise_states='stored' describes, bitwise"""
    dn = device_noise(2, True, seed=5).asdict()
    runs = []
    for name, kw in (('states', dict(train_noise_states='stored')), ('exact', dict(train_device_noise_exact='stored')),
                     ('both', dict(train_device_noise_exact='stored', train_noise_states='stored'))):
        s, hist, _ = _run(tmp_path, name, dev, n=2, net_size=[2, 1, 2, 1], train_device_noise=dn, **kw)
        assert s.trainer.noise_states == 'stored'
        runs.append((hist['loss_steps'], H.flat(s.model).clone()))
    for other in runs[1:]:
        assert runs[0][0] == other[0] and torch.equal(runs[0][1], other[1])


def test_refusals(dev, tmp_path):
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import NoiseModel, Sampling
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    from quanonet_amd.solver import DataParallelTrainer, PTSolver
    from quanonet_amd.sweep import SweepSolver
    data = _data()
    quiet = lambda *a, **k: None
    dn = _past_noise(7)
    solver = lambda name, **kw: PTSolver(_cfg(tmp_path, name, **kw), data, device=dev, log=quiet)
    with pytest.raises(ValueError, match="'stored' needs train_device_noise"):
        solver('alone', train_device_noise_exact='stored')
    with pytest.raises(ValueError, match='train_noise'):
        solver('uniform', train_noise=NoiseModel(p1=0.01), train_device_noise_exact='stored')
    sp = Sampling(trajectories=8, seed=1)
    for key in ('train_sampling', 'train_trajectories', 'train_jump_trajectories'):
        with pytest.raises(ValueError, match=f"'stored' does not combine with {key}"):
            solver(key, train_device_noise=dn, train_device_noise_exact='stored', **{key: sp})
    with pytest.raises(ValueError, match="absent or 'stored'"):
        solver('states', train_device_noise=dn, train_device_noise_exact='stored', train_noise_states='inverse')
    with pytest.raises(ValueError, match='n <= 9'):
        solver('n10', n=10, train_device_noise=device_noise(10, True, seed=5, scale=0.5), train_device_noise_exact='stored')
    # a refused model: the layer amplification and the bound are named
    with pytest.raises(ValueError, match=r'for one layer; the stored-state walk.s bound is 7'):
        solver('layer', train_device_noise=dict(dn.asdict(), p2=[0.9] * 7), train_device_noise_exact='stored')
    with pytest.raises(ValueError, match='A_dev = inf'):                    # a singular channel
        solver('singular', train_device_noise=dict(dn.asdict(), p1=[0.75] * 7), train_device_noise_exact='stored')
    # the two raises the inverse value keeps
    with pytest.raises(ValueError, match="None or 'wide'"):
        solver('value', train_device_noise=dn, train_device_noise_exact='tiled')
    with pytest.raises(ValueError, match='does not exist on tiles'):
        solver('wide-states', train_device_noise=device_noise(7, True, seed=5, scale=0.5), train_device_noise_exact='wide',
               train_noise_states='stored')
    # a non-fused model or optimizer
    m = _model('quanonet', 7, True, 'Z').to(dev)
    with pytest.raises(ValueError, match='fused'):
        DataParallelTrainer(m, fused=False, train_device_noise=dn, train_device_noise_exact='stored')
    with pytest.raises(ValueError, match='fused'):
        DataParallelTrainer(m, optimizer='sgd', train_device_noise=dn, train_device_noise_exact='stored')
    # the four member solvers
    for cls in (EnsembleSolver, SweepSolver, DepthSweepSolver, QubitSweepSolver):
        cfgs = [_cfg(tmp_path, cls.__name__, n=2, net_size=[2, 1, 2, 1], seed=k, run_id=f'm{k}') for k in (0, 1)]
        cfgs[1]['train_device_noise_exact'] = 'stored'
        with pytest.raises(ValueError, match='train_device_noise_exact'):
            cls(cfgs, data, device=dev, log=quiet)
