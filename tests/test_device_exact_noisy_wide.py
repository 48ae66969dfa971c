"""
The exact forward under a calibrated device noise model at n = 7..9 (qhea_model_forward_noisy_device_exact_wide,
quanonet_amd.noise.device_exact_noisy_predict, evaluate_noisy(exact='device')): the per-wire channel sites of
hea_density_device.hip on the tiles of hea_density_wide.hip.  On the GPU: against the literal Kraus timeline in numpy
(tests/device_noise_reference.py, which is generic in n and so checks the host fold into four sites per wire as well), the stage
edges, idle on / off, the closing pair, the readout of the top bit, the uniform setting against the uniform tiled call, the
default setting against the ideal forward, determinism and chunk independence, errors, the grid guard, graph capture and the
launch count, the solvers, the quantum-jump kernels against it.  Without a GPU: symbols, version, workspace size, the return
codes in device_call_check's order and the stage-B wire map restated in numpy.  Tolerance against the references: atol 1e-10,
the one the HIP path is held to against the oracle.

A reference evolution is computed once per circuit and shared among the read-outs that differ only in the basis change and the
value table (_final_rho); 5 s per sub-layer for two rows at n = 9, which sets the depths used here.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import device_noise_reference as R
from tests import device_wide_precision_cases as DW
from tests import helpers as H
from tests.test_device_noise_training_abi import as_dict
from tests.test_exact_noisy_wide import _is_kernel, _pass_wires
from tests.test_noisy_forward import _circuit, _ideal, _inputs, _solver_data

gpu = pytest.mark.gpu
ATOL = 1e-10
SIZE, CALL = 'qhea_model_device_exact_noisy_wide_workspace_bytes', 'qhea_model_forward_noisy_device_exact_wide'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


# ---- without a GPU -------------------------------------------------------------------------------------------------------------

def _record(n, **kw):
    """a DeviceNoiseParams with n_wires = n whose arrays the caller may overwrite"""
    from quanonet_amd.noise import DeviceNoise
    return DeviceNoise(p1=0.01, p2=0.02, readout01=0.01, readout10=0.03, t1=100.0, t2=80.0, t_rx=0.05, t_rot=0.05, t_cx=0.3,
                       **kw).params(n)


def test_abi_checks_without_a_device():
    """symbols, version, the workspace size, and the return codes that need no device in device_call_check's order: the
    descriptor, the setting (null, n_wires, t2 > 2 t1, a rate outside [0, 1]), then the qubit range"""
    from quanonet_amd import _lib
    lib = _lib.load()
    assert lib.qhea_version() >= 640 and _lib.MIN_LIB_VERSION >= 640
    for name in (SIZE, CALL):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    size, call, uniform = getattr(lib, SIZE), getattr(lib, CALL), lib.qhea_model_exact_noisy_wide_workspace_bytes
    none = (None,) * 4
    for n in (7, 8, 9):
        d = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
        for batch in (0, 1, 100, 3000):
            assert size(ctypes.byref(d), batch) == uniform(ctypes.byref(d), batch) > batch * 4 ** n * 16
        assert size(ctypes.byref(d), -1) == 0
        ok = _record(n)
        assert call(ctypes.byref(d), 0, *none, ctypes.byref(ok), None, None, None, 0, None) == 0         # an empty batch
        assert call(ctypes.byref(d), -1, *none, ctypes.byref(ok), None, None, None, 0, None) == -1
        assert call(ctypes.byref(d), 10, *none, ctypes.byref(ok), None, None, None, 0, None) == -1       # no pointers
        assert call(None, 10, *none, ctypes.byref(ok), None, None, None, 0, None) == -1                  # no descriptor
    assert size(None, 100) == 0
    for n in (6, 10):
        d = _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
        assert size(ctypes.byref(d), 100) == 0
    # the order: every bad setting is QHEA_EINVAL at a qubit count the call does not serve, a good one QHEA_EUNSUPPORTED there
    for n in (2, 6, 10, 12, 7, 9):
        d = _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
        bad = [None, ctypes.byref(_record(n + 1 if n < 12 else n - 1))]                                  # null; n_wires != n
        rec = _record(n)
        rec.t2[n - 1] = 2.0 * rec.t1[n - 1] + 1.0
        bad.append(ctypes.byref(rec))
        for name, value in (('p1', -0.01), ('p2', 1.5), ('readout01', 2.0), ('readout10', float('nan'))):
            rec = _record(n)
            getattr(rec, name)[n - 1] = value
            bad.append(ctypes.byref(rec))
        for b in bad:
            assert call(ctypes.byref(d), 10, *none, b, None, None, None, 0, None) == -1, n
        want = -1 if n in (7, 9) else -2                                 # in range: the next refusal is the missing pointers
        assert call(ctypes.byref(d), 10, *none, ctypes.byref(_record(n)), None, None, None, 0, None) == want, n


def _stage_b_global(n, local):
    """hea_density_device_wide.hip's global_wire<N, 1>: local 0, 1 -> global 0, 1, local w >= 2 -> w + n - 6"""
    return local if local < 2 else local + n - 6


@pytest.mark.parametrize('n', [7, 8, 9])
def test_stage_wire_maps(n):
    """every slot j's target-site and control-site wires are the wires Pass<6, .> of its stage serves, under the compile-time
    local -> global maps of the two stages; after test_exact_noisy_wide.test_tile_maps"""
    wires_b = [_stage_b_global(n, l) for l in range(6)]
    assert wires_b == [0, 1, n - 4, n - 3, n - 2, n - 1]                 # the tile map of stage B, as test_tile_maps checks it
    seen = []
    for j in range(n):                                                   # slot j: target j (kTgt site), control j + 1 mod n (kCtl)
        stage, J = ('A', j) if j < 5 else ('B', j - n + 6)
        assert 0 <= J <= 5
        t, c = _pass_wires(J)
        glob = (lambda l: l) if stage == 'A' else (lambda l: _stage_b_global(n, l))
        assert (glob(t), glob(c)) == (j, (j + 1) % n), (n, j)
        # pending gates: pass 0 wire 0's, every pass j <= n - 2 wire j + 1's (the kEnc / kRot sites of those wires)
        seen += ([glob(t)] if j == 0 else []) + ([glob(c)] if j <= n - 2 else [])
        # the record of a stage is indexed by local wire and local pass: slot of local pass J
        assert (J if stage == 'A' else J + n - 6) == j
    assert seen == list(range(n))                                        # every wire's gates exactly once, in wire order
    # the one-qubit stages: stage A serves local = global 0..5, stage B the local wires >= 12 - n, global 6..n-1
    assert [_stage_b_global(n, l) for l in range(12 - n, 6)] == list(range(6, n))


# ---- helpers of the GPU part ---------------------------------------------------------------------------------------------------

def _predict(m, inputs, dn, **kw):
    from quanonet_amd.noise import device_exact_noisy_predict
    p, sd = device_exact_noisy_predict(m, inputs, dn, **kw)
    torch.cuda.synchronize()
    return p[:, 0].cpu().numpy(), sd.cpu().numpy()


def _net_model(kind, n, net, readout, seed=0, trainable=True):
    """tests.test_noisy_forward._model with the net given"""
    kw = dict(if_trainable_freq=trainable, scale_coeff=0.7, ham_bound=(-2.0, 3.0))
    if readout == 'diag':
        kw['ham_diag'] = np.random.default_rng(seed + 50).normal(size=1 << n)
    else:
        kw['ham_pauli'] = readout
    m = H.quanonet(n, 3, 2, net, seed, **kw) if kind == 'quanonet' else H.heaqnn(n, 4, net, seed, **kw)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(seed + 7)
        for name, p in m.named_parameters():
            if name.endswith('freq.weights'):
                p.copy_(0.5 + torch.rand(p.shape, generator=gen, dtype=torch.float64))
    return m


_RHO = {}


def _final_rho(c, nz, rows):
    """the reference's rho of the first `rows` rows before the basis change, once per circuit, weights, inputs and setting"""
    x = np.ascontiguousarray(c['x'][:rows])
    key = (c['n'], repr(c['cfgs']), x.tobytes(), np.ascontiguousarray(c['w']).tobytes(), repr(sorted(nz.items())))
    if key not in _RHO:
        rho = R.final_rho(c['n'], c['cfgs'], c['x'][:rows], c['w'], nz, 'Z')
        rho.setflags(write=False)
        _RHO[key] = rho
    return _RHO[key]


def _reference(c, dn, rows):
    """(mean, std) of the first `rows` rows by the Kraus timeline"""
    n = c['n']
    nz = as_dict(dn, n)
    rho = _final_rho(c, nz, rows)
    rho = np.ascontiguousarray(R.basis_change(rho.reshape((-1,) + (2,) * (2 * n)), n, c['ham_pauli'])).reshape(-1, 1 << n, 1 << n)
    mean, var = R.moments_of(np.real(np.einsum('bkk->bk', rho)), n, nz, c['offset'], c['coeff'], c['ham_diag'])
    return mean, np.sqrt(np.maximum(var, 0.0))


def _compare(m, ins, dn, k, tag):
    """the GPU's pred and shot_std of all rows against the reference on the first k; returns the GPU's"""
    c, bias = _circuit(m, ins)
    pred, sd = _predict(m, ins, dn)
    mean, std = _reference(c, dn, k)
    print(f'{tag}: max|pred err|={np.abs(pred[:k] - mean - bias).max():.2e} max|std err|={np.abs(sd[:k] - std).max():.2e}')
    np.testing.assert_allclose(pred[:k] - bias, mean, rtol=0, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(sd[:k], std, rtol=0, atol=ATOL, err_msg=tag)
    assert np.all(np.isfinite(pred)) and np.all(np.isfinite(sd)) and np.all(sd >= 0.0)
    return pred, sd


# ---- 1. against the reference --------------------------------------------------------------------------------------------------

# both kinds see a sub-layer with and one without the encoding, and a second block (the column offset); two sub-layers at n = 9
NETS = {('quanonet', 7): (1, 2, 1, 1), ('quanonet', 8): (1, 2, 1, 1), ('quanonet', 9): (1, 1, 1, 1),
        ('heaqnn', 7): (2, 2), ('heaqnn', 8): (2, 2), ('heaqnn', 9): (1, 2)}


@gpu
@pytest.mark.parametrize('readout', ['Z', 'X', 'Y', 'diag'])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
@pytest.mark.parametrize('n', [7, 8, 9])
def test_against_the_reference(dev, n, kind, readout):
    """the per-wire setting in which no two wires and no two ring slots agree (device_wide_precision_cases.perwire_setting): a
    wire-index mix-up shows"""
    rows = 3 if n < 9 else 2
    m = _net_model(kind, n, NETS[kind, n], readout, seed=n).to(dev)
    ins = _inputs(kind, rows, dev, seed=rows)
    _compare(m, ins, DW.perwire_setting(n), 2, f'n={n} {kind} {readout}')


# ---- 2. stage edges ------------------------------------------------------------------------------------------------------------

def _edge_model(shape, n, readout):
    """a QuanONet's net is (branch depth, LD, trunk depth, LD) and its circuit runs the trunk blocks first, then the branch blocks
    (oracle.hea_oracle.block_configs_quanonet): the shape names say where the blocks without sub-layers come in the circuit"""
    kw = dict(if_trainable_freq=True, scale_coeff=0.7, ham_bound=(-2.0, 3.0), ham_pauli=readout)
    if shape == 'heaqnn-ld0':
        return 'heaqnn', H.heaqnn(n, 4, (2, 0), 3, **kw)                 # encoding blocks only
    if shape == 'ld0-last':
        return 'quanonet', H.quanonet(n, 3, 2, (2, 0, 1, 2), 3, **kw)    # circuit (n, 2), (n, 0), (n, 0): ring stages first
    if shape == 'ld0-first':
        return 'quanonet', H.quanonet(n, 3, 2, (1, 1, 2, 0), 3, **kw)    # circuit (n, 0), (n, 0), (n, 1): the first stage of the
                                                                         # circuit, the one that loads nothing, is a one-qubit stage
    return 'heaqnn', H.heaqnn(n, 4, (1, 1), 3, **kw)                     # one sub-layer


@gpu
@pytest.mark.parametrize('shape', ['heaqnn-ld0', 'ld0-last', 'ld0-first', 'one-sublayer'])
@pytest.mark.parametrize('n', [7, 9])
def test_stage_edges(dev, n, shape):
    k = 2 if n == 7 else 1
    from oracle import hea_oracle as O
    assert [ld for _, ld in O.block_configs_quanonet(n, (2, 0, 1, 2))] == [2, 0, 0]        # what 'ld0-last' and 'ld0-first' mean
    assert [ld for _, ld in O.block_configs_quanonet(n, (1, 1, 2, 0))] == [0, 0, 1]
    for readout in ('Z', 'Y'):
        kind, m = _edge_model(shape, n, readout)
        m = m.to(dev)
        ins = _inputs(kind, 2, dev, seed=n)
        _compare(m, ins, DW.perwire_setting(n), k, f'n={n} {shape} {readout}')


# ---- 3. what the device model adds over the uniform one ------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n', [7, 9])
def test_idle_on_and_off(dev, n):
    """the idle decay of the ring (folded into the kRot and kTgt sites): the two results differ and each matches its reference"""
    m = _net_model('heaqnn', n, (1, 1), 'Z', seed=n + 1).to(dev)
    ins = _inputs('heaqnn', 2, dev, seed=n)
    strong = dict(p1=0.01, p2=0.03, t1=tuple(4.0 + q for q in range(n)), t2=tuple(3.0 + 1.5 * q for q in range(n)), t_rx=0.05,
                  t_rot=0.1, t_cx=0.3)
    from quanonet_amd.noise import DeviceNoise
    out = {}
    for idle in (True, False):
        out[idle] = _compare(m, ins, DeviceNoise(idle=idle, **strong), 1, f'n={n} idle={idle}')
    assert np.abs(out[True][0] - out[False][0]).min() > 1e-3, out


@gpu
@pytest.mark.parametrize('n', [7, 8, 9])
def test_closing_pair(dev, n):
    """relaxation on wire n-1 and wire 0 only, no gate errors: the closing slot (n-1, 0) is the local pair (5, 0) of stage B"""
    from quanonet_amd.noise import DeviceNoise
    inf = math.inf
    t1 = (2.0,) + (inf,) * (n - 2) + (3.0,)
    t2 = (1.5,) + (inf,) * (n - 2) + (4.0,)
    dn = DeviceNoise(t1=t1, t2=t2, t_rx=0.05, t_rot=0.1, t_cx=0.3, idle=True)
    m = _net_model('heaqnn', n, (1, 1), 'X', seed=n + 2).to(dev)
    ins = _inputs('heaqnn', 2, dev, seed=n)
    pred, _ = _compare(m, ins, dn, 1, f'n={n} closing pair')
    ideal = _ideal(m, ins).cpu().numpy()
    assert np.abs(pred - ideal).max() > 1e-3                             # the two wires' relaxation shows (in some row)


@gpu
@pytest.mark.parametrize('n', [7, 8, 9])
def test_readout_of_the_top_bit(dev, n):
    """readout01 != readout10 on bit n-1 alone and no other noise: a bit-index error of the value tables above bit 5 shows.
    The state is the ideal one, so the reference is the oracle's state with the confusion of that bit"""
    from oracle import hea_oracle as O
    from quanonet_amd.noise import DeviceNoise
    r01 = (0.0,) * (n - 1) + (0.15,)
    r10 = (0.0,) * (n - 1) + (0.05,)
    dn = DeviceNoise(readout01=r01, readout10=r10)
    for readout in ('Z', 'diag'):
        m = _net_model('quanonet', n, (1, 1, 1, 1), readout, seed=n + 3).to(dev)
        ins = _inputs('quanonet', 2, dev, seed=n)
        c, bias = _circuit(m, ins)
        pred, sd = _predict(m, ins, dn)
        psi = O.hea_state(c['n'], c['cfgs'], c['x'], c['w'])
        prob = psi.real ** 2 + psi.imag ** 2
        mean, var = R.moments_of(prob, n, as_dict(dn, n), c['offset'], c['coeff'], c['ham_diag'])
        np.testing.assert_allclose(pred - bias, mean, rtol=0, atol=ATOL)
        np.testing.assert_allclose(sd, np.sqrt(np.maximum(var, 0.0)), rtol=0, atol=ATOL)
        swapped = R.moments_of(prob, n, as_dict(DeviceNoise(readout01=r10, readout10=r01), n), c['offset'], c['coeff'],
                               c['ham_diag'])[0]
        assert np.abs(swapped - mean).max() > 1e-4                       # the asymmetry is resolved (in some row)


@gpu
@pytest.mark.parametrize('n', [7, 8, 9])
def test_uniform_setting_is_the_uniform_call(dev, n):
    from quanonet_amd.noise import DeviceNoise, NoiseModel, wide_exact_noisy_predict
    nm = NoiseModel(p1=0.03, p2=0.08, readout=0.04)
    for kind, readout in (('quanonet', 'Y'), ('heaqnn', 'diag')):
        m = _net_model(kind, n, (2, 1, 1, 2) if kind == 'quanonet' else (3, 1), readout, seed=n).to(dev)
        ins = _inputs(kind, 5, dev, seed=5)
        pred, sd = _predict(m, ins, DeviceNoise.uniform(nm))
        p, s = wide_exact_noisy_predict(m, ins, nm)
        print(f'n={n} {kind}: {np.abs(pred - p[:, 0].cpu().numpy()).max():.2e} {np.abs(sd - s.cpu().numpy()).max():.2e}')
        np.testing.assert_allclose(pred, p[:, 0].cpu().numpy(), rtol=0, atol=ATOL)
        np.testing.assert_allclose(sd, s.cpu().numpy(), rtol=0, atol=ATOL)


@gpu
@pytest.mark.parametrize('n', [7, 8, 9])
def test_default_setting_is_the_ideal_forward(dev, n):
    from quanonet_amd.noise import DeviceNoise
    for kind, readout in (('quanonet', 'X'), ('heaqnn', 'Z')):
        m = _net_model(kind, n, (2, 1, 1, 2) if kind == 'quanonet' else (3, 1), readout, seed=n).to(dev)
        ins = _inputs(kind, 5, dev, seed=5)
        pred, _ = _predict(m, ins, DeviceNoise())
        np.testing.assert_allclose(pred, _ideal(m, ins).cpu().numpy(), rtol=0, atol=ATOL)


@gpu
@pytest.mark.parametrize('n,rows', [(7, 1), (7, 3), (9, 1)])
def test_small_batches(dev, n, rows):
    m = _net_model('quanonet', n, (1, 1, 1, 1), 'X', seed=n + 1).to(dev)
    ins = _inputs('quanonet', rows, dev, seed=n)
    _compare(m, ins, DW.perwire_setting(n), min(rows, 2 if n == 7 else 1), f'n={n} rows={rows}')


# ---- 4. determinism, chunking, routing -----------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n,kind,rows,chunk', [(7, 'quanonet', 300, 7), (9, 'heaqnn', 5, 2)])
def test_deterministic_and_chunk_independent(dev, n, kind, rows, chunk):
    m = _net_model(kind, n, (2, 1, 1, 2) if kind == 'quanonet' else (2, 1), 'Z', seed=2).to(dev)
    ins = _inputs(kind, rows, dev, seed=3)
    dn = DW.perwire_setting(n)
    a, sa = _predict(m, ins, dn)
    b, sb = _predict(m, ins, dn)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    c, sc = _predict(m, ins, dn, chunk_rows=chunk)
    assert np.array_equal(a, c) and np.array_equal(sa, sc)
    lo = rows * 3 // 10
    hi = lo + max(1, min(37, rows // 4))
    p, s = _predict(m, tuple(t[lo:hi] for t in ins), dn)                 # a slice of the rows is the same rows of the whole call
    assert np.array_equal(p, a[lo:hi]) and np.array_equal(s, sa[lo:hi])


@gpu
def test_python_routing(dev):
    from quanonet_amd.noise import DeviceNoise, NoiseModel, device_exact_noisy_predict, exact_noisy_predict
    dn5 = DW.perwire_setting(5)
    m = _net_model('quanonet', 5, (2, 1, 1, 2), 'Z', seed=2).to(dev)
    ins = _inputs('quanonet', 100, dev, seed=3)
    for kw in ({}, {'chunk_rows': 33}):
        p, s = exact_noisy_predict(m, ins, dn5)
        wp, ws = device_exact_noisy_predict(m, ins, dn5, **kw)
        assert torch.equal(p, wp) and torch.equal(s, ws)
    ins4 = _inputs('heaqnn', 4, dev)
    with pytest.raises(ValueError, match='device_noisy_predict'):
        device_exact_noisy_predict(_net_model('heaqnn', 10, (1, 1), 'Z').to(dev), ins4, DW.perwire_setting(10))
    m8 = _net_model('heaqnn', 8, (1, 1), 'Z').to(dev)
    with pytest.raises(ValueError, match='wide_exact_noisy_predict.*DeviceNoise.uniform'):
        device_exact_noisy_predict(m8, ins4, NoiseModel(p1=0.01))
    with pytest.raises(ValueError, match='8 wires'):                     # a setting of another size
        device_exact_noisy_predict(m8, ins4, DW.perwire_setting(7))
    p, sd = device_exact_noisy_predict(m8, ins4, DeviceNoise())
    assert p.shape == (4, 1) and sd.shape == (4,)


# ---- 5. errors launch nothing --------------------------------------------------------------------------------------------------

@gpu
def test_errors_launch_nothing(dev):
    from quanonet_amd import _lib
    lib = _lib.load()
    m = _net_model('quanonet', 7, (1, 1, 1, 1), 'Z').to(dev)
    ins = _inputs('quanonet', 10, dev)
    desc, params = m.fused_desc(), H.flat(m)
    out = torch.full((10,), 123.0, dtype=torch.float64, device=dev)
    sd = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    ok = DW.perwire_setting(7).params(7)
    bad = _record(7)
    bad.p2[3] = 1.5
    with pytest.raises(_lib.QheaError):
        _lib.model_forward_noisy_device_exact_wide(desc, ins[0], ins[1], params, bad, out=out, shot_std=sd)
    with pytest.raises(_lib.QheaError):                                  # n_wires != n
        _lib.model_forward_noisy_device_exact_wide(desc, ins[0], ins[1], params, _record(8), out=out, shot_std=sd)
    for n in (6, 10):
        mo = _net_model('heaqnn', n, (1, 1), 'Z').to(dev)
        io = _inputs('heaqnn', 10, dev)
        with pytest.raises(_lib.Unsupported):
            _lib.model_forward_noisy_device_exact_wide(mo.fused_desc(), io[0], None, H.flat(mo), _record(n), out=out, shot_std=sd)
    need = getattr(lib, SIZE)(ctypes.byref(desc), 10)
    assert need >= 10 * (4 ** 7) * 16
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args = [ctypes.byref(desc), 10, _lib._ptr(ins[0]), _lib._ptr(ins[1]), _lib._ptr(params), None, ctypes.byref(ok),
            _lib._ptr(out), _lib._ptr(sd), _lib._ptr(ws)]
    with torch.cuda.device(dev):
        assert getattr(lib, CALL)(*args, need - 1, _lib._stream(dev)) == -3
        assert getattr(lib, CALL)(*args[:-1], None, need, _lib._stream(dev)) == -3
    torch.cuda.synchronize()
    assert torch.all(out == 123.0) and torch.all(sd == 456.0)
    # shot_std is optional
    pred, none = _lib.model_forward_noisy_device_exact_wide(desc, ins[0], ins[1], params, ok)
    both, _ = _lib.model_forward_noisy_device_exact_wide(desc, ins[0], ins[1], params, ok, shot_std=sd)
    torch.cuda.synchronize()
    assert none is None and torch.equal(pred, both) and torch.all(sd != 456.0)


@gpu
@pytest.mark.parametrize('n', [7, 8, 9])
def test_grid_guard(dev, n):
    """test_exact_noisy_wide.test_grid_guard for this call: the first batch whose rows x 4^(n-6) workgroups pass INT_MAX is a
    bad argument before the workspace is looked at; the workspace holds one row, so the largest batch admitted answers -3"""
    from quanonet_amd import _lib
    lib = _lib.load()
    m = _net_model('heaqnn', n, (1, 1), 'Z').to(dev)
    ins = _inputs('heaqnn', 2, dev)
    desc, params = m.fused_desc(), H.flat(m)
    out = torch.full((2,), 123.0, dtype=torch.float64, device=dev)
    sd = torch.full((2,), 456.0, dtype=torch.float64, device=dev)
    ok = DW.perwire_setting(n).params(n)
    need = getattr(lib, SIZE)(ctypes.byref(desc), 1)
    assert need >= (4 ** n) * 16
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    limit = (2 ** 31 - 1) >> (2 * (n - 6))

    def call(batch):
        return getattr(lib, CALL)(ctypes.byref(desc), batch, _lib._ptr(ins[0]), None, _lib._ptr(params), None, ctypes.byref(ok),
                                  _lib._ptr(out), _lib._ptr(sd), _lib._ptr(ws), need, _lib._stream(dev))
    with torch.cuda.device(dev):
        assert call(limit + 1) == -1
        assert call(limit) == -3
    torch.cuda.synchronize()
    _lib.check_status(dev)
    assert torch.all(out == 123.0) and torch.all(sd == 456.0)


# ---- 6. graph capture and launch count -----------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n', [7, 9])
@pytest.mark.parametrize('readout', ['Z', 'X'])
def test_graph_capturable_launch_count(dev, n, readout):
    """prep, value tables, 2 x sub-layers + 2 x blocks without sub-layers + 2 for X / Y, read-out; relaxation adds no launch"""
    from quanonet_amd import _lib
    rows = 5
    nz = DW.perwire_setting(n).params(n)
    for m, kind, sublayers, ld0 in ((_net_model('quanonet', n, (2, 1, 1, 2), readout), 'quanonet', 4, 0),
                                    (_net_model('quanonet', n, (2, 0, 1, 2), readout), 'quanonet', 2, 2)):
        m = m.to(dev)
        ins = _inputs(kind, rows, dev)
        desc, params = m.fused_desc(), H.flat(m)
        out = torch.empty(rows, dtype=torch.float64, device=dev)
        sd = torch.empty(rows, dtype=torch.float64, device=dev)
        call = lambda: _lib.model_forward_noisy_device_exact_wide(desc, ins[0], ins[1], params, nz, out=out, shot_std=sd)
        call()                                                           # sizes the workspace outside the capture
        torch.cuda.synchronize()
        eager = (out.clone(), sd.clone())
        launches = H.kernel_launches(dev, call)
        stages = [k for k in launches if _is_kernel(k[0], 'density_dev_wide_ring_kernel', n) or
                  _is_kernel(k[0], 'density_dev_wide_wires_kernel', n)]
        others = [k[0] for k in launches if k not in stages]
        assert len(stages) == 2 * sublayers + 2 * ld0 + (2 if readout == 'X' else 0), [k[0] for k in launches]
        assert sum(_is_kernel(k[0], 'density_dev_wide_ring_kernel', n) for k in stages) == 2 * sublayers
        for k in stages:
            assert k[1] == (rows * 4 ** (n - 6), 1, 1) and k[2] == (256, 1, 1), k
        assert len(others) == 3 and 'prep_model_kernel' in others[0] and \
            _is_kernel(others[1], 'density_dev_wide_values_kernel', n) and \
            _is_kernel(others[2], 'density_wide_readout_kernel', n), others
        assert launches[-1][0] == others[2] and [k[0] for k in launches[:2]] == others[:2]
        torch.cuda.synchronize()
        # kernel_launches captures and reads the nodes but replays nothing: instantiate a graph of the call and replay it into
        # poisoned outputs (the capture itself runs no kernel, so only the replay can write them)
        out.fill_(float('nan'))
        sd.fill_(float('nan'))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                call()
            torch.cuda.synchronize()
            assert torch.isnan(out).all() and torch.isnan(sd).all()      # captured, not run
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(sd, eager[1])
        out.fill_(float('nan'))
        sd.fill_(float('nan'))
        g.replay()                                                       # a second replay of the same nodes
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(sd, eager[1])


# ---- 7. solvers ----------------------------------------------------------------------------------------------------------------

@gpu
def test_solver_evaluate_noisy_device(dev, tmp_path):
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import NoiseModel, Sampling, device_exact_noisy_predict
    from quanonet_amd.solver import PTSolver, regression_metrics
    data = _solver_data()
    cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': 7, 'net_size': [2, 1, 2, 1], 'scale_coeff': 0.01,
           'if_trainable_freq': 'true', 'learning_rate': 1e-2, 'batch_size': 100, 'num_epochs': 2, 'seed': 0,
           'prefix': str(tmp_path / 'solo'), 'run_id': 'r0', 'eval_batch_size': 64}
    quiet = lambda *a, **k: None
    s = PTSolver(cfg, data, device=dev, log=quiet)
    hist = s.train()
    s.evaluate(hist)
    mpath = os.path.join(s.out_dir, 'metric.json')
    before = (open(mpath).read(), os.stat(mpath).st_mtime_ns)
    files = set(os.listdir(s.out_dir))
    dn = DW.perwire_setting(7)
    y_true = torch.tensor(data['test_output'], device=dev)
    res = s.evaluate_noisy(dn, exact='device')
    assert set(os.listdir(s.out_dir)) == files
    pred, sd = device_exact_noisy_predict(s.model, s.test_input, dn)
    for k, v in regression_metrics(pred, y_true).items():
        assert res[k] == v, k
    assert res['exact'] is True and res['mean_shot_std'] == float(sd.mean().item()) and res['noise'] == dn.asdict()
    assert 'mean_stderr' not in res and 'sampling' not in res
    res2 = s.evaluate_noisy(dn, out_name='device_metric.json', exact='device')
    assert set(os.listdir(s.out_dir)) == files | {'device_metric.json'}
    with open(os.path.join(s.out_dir, 'device_metric.json')) as f:
        assert json.load(f) == json.loads(json.dumps(res2))
    with pytest.raises(ValueError, match="'tiled'.*'wide'.*'device'|'wide'.*'device'.*'tiled'"):      # names what it takes
        s.evaluate_noisy(dn, exact='tiled')
    with pytest.raises(ValueError, match='sampling='):
        s.evaluate_noisy(dn, exact='device', sampling=Sampling(seed=1))
    with pytest.raises(ValueError, match='DeviceNoise'):
        s.evaluate_noisy(NoiseModel(p1=0.01), exact='device')
    assert (open(mpath).read(), os.stat(mpath).st_mtime_ns) == before and \
        set(os.listdir(s.out_dir)) == files | {'device_metric.json'}
    ens = EnsembleSolver([dict(cfg, seed=k, run_id=f'm{k}', prefix=str(tmp_path / 'ens')) for k in (0, 1)], data, device=dev,
                         log=quiet)
    ens.train()
    outs = ens.evaluate_noisy(dn, exact='device')
    assert len(outs) == 2
    for mem, o in zip(ens.members, outs):
        p, _ = device_exact_noisy_predict(mem.model, mem.test_input, dn)
        assert o['exact'] is True and o['MSE'] == regression_metrics(p, y_true)['MSE']
        assert not os.path.exists(os.path.join(mem.out_dir, 'metric.json'))


# ---- 8. the quantum-jump kernels against the exact value -----------------------------------------------------------------------

def _strong(n):
    """all wires different; t_cx / T1 in [0.15, 0.3], so that jumps fire in most trajectories (test_device_traj._strong(n, True,
    seed=2), restated so that this file does not import that module's fixtures)"""
    from quanonet_amd.noise import DeviceNoise
    rng = np.random.default_rng(2000 + 10 * n + 2)
    t1 = rng.uniform(1.0, 2.0, n)
    return DeviceNoise(p1=rng.uniform(0.02, 0.05, n), p2=rng.uniform(0.05, 0.1, n), readout01=rng.uniform(0.01, 0.05, n),
                       readout10=rng.uniform(0.04, 0.09, n), t1=t1, t2=t1 * rng.uniform(0.5, 2.0, n), t_rx=0.05, t_rot=0.1,
                       t_cx=0.3, idle=True)


@gpu
@pytest.mark.parametrize('n', [7, 8, 9])
@pytest.mark.parametrize('shots', [0, 20000])
def test_jump_kernel_against_exact(dev, n, shots):
    """
    test_exact_noisy_wide.test_trajectory_kernel_against_exact for the quantum-jump kernels of hea_noise_device.hip at
    n = 7..9, which had no exact value to be held against on the GPU.  The bound is a condition on a correct kernel, not a
    measurement: the estimator is unbiased, the seeds are fixed here, and over the 96 compared values a correct kernel leaves
    5 stderr with probability about 5e-5.
    The n = 7 stream was replayed on the CPU first at the full T = 20000 (device_traj_reference.replay_values, rows 0 and 1,
    against device_noise_reference.device_moments): seed 1007, largest |z| 0.96 in expectation mode and 1.36 in shot mode,
    shot-mode stderr sqrt(S) / shot_std within [0.992, 1.006].
    """
    from quanonet_amd.noise import Sampling, device_noisy_predict
    from tests.test_noisy_forward import _model
    m = _model('heaqnn', n, True, 'Z', seed=n + 20).to(dev)
    ins = _inputs('heaqnn', 16, dev, seed=n)
    dn = _strong(n)
    p, se = device_noisy_predict(m, ins, dn, Sampling(shots=shots, trajectories=20000, seed=1000 + n))
    torch.cuda.synchronize()
    pred, se = p[:, 0].cpu().numpy(), se.cpu().numpy()
    exact, sd = _predict(m, ins, dn)
    assert np.all(se > 0)
    print(f'n={n} shots={shots}: z={(pred - exact) / se}')
    assert np.all(np.abs(pred - exact) < 5 * se), (pred - exact) / se
    if shots:
        print(f'stderr sqrt(S) / shot_std = {se * np.sqrt(shots) / sd}')
        assert np.all(np.abs(se * np.sqrt(shots) / sd - 1.0) < 0.1), se * np.sqrt(shots) / sd
