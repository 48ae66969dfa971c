"""
The exact noisy forward at n = 7..9 (qhea_model_forward_noisy_exact_wide, quanonet_amd.noise.wide_exact_noisy_predict,
evaluate_noisy(exact='wide')): the density matrix in device memory, six wires at a time in LDS.  On the GPU: against the numpy
density matrix (tests/density_reference.py), noiseless = ideal, the stage edges, determinism and chunk independence, errors, the grid guard,
graph capture and the launch count, the wide trajectory kernels against it, the solvers.  Without a GPU: the two tile index
maps restated in numpy.  Tolerance against the references: atol 1e-10, the one the HIP path is held to against the oracle.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from tests import density_reference as DR
from tests import helpers as H
from tests import noise_oracle as NO
from tests.test_noisy_forward import _circuit, _ideal, _inputs, _model, _noisy, _solver_data

gpu = pytest.mark.gpu
ATOL = 1e-10
NOISES = ((0.03, 0.08, 0.04), (0.003, 0.008, 0.004))
WORST = {}                                                               # (test, n) -> largest error seen so far


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _wide(m, inputs, noise, **kw):
    from quanonet_amd.noise import wide_exact_noisy_predict
    p, sd = wide_exact_noisy_predict(m, inputs, noise, **kw)
    torch.cuda.synchronize()
    return p[:, 0].cpu().numpy(), sd.cpu().numpy()


def _reference(c, p1, p2, q, rows):
    mean, var = DR.exact_moments(c['n'], c['cfgs'], c['x'][:rows], c['w'], p1, p2, q, c['offset'], c['coeff'], c['ham_diag'],
                                 c['ham_pauli'])
    return mean, np.sqrt(np.maximum(var, 0.0))


def _worst(test, n, *errs):
    WORST[test, n] = max(WORST.get((test, n), 0.0), *[float(np.abs(e).max()) for e in errs])
    print(f'{test} n={n}: largest error so far {WORST[test, n]:.2e}')


def _against_reference(m, ins, c, bias, settings, k, tag, n):
    from quanonet_amd.noise import NoiseModel
    for p1, p2, q in settings:
        pred, sd = _wide(m, ins, NoiseModel(p1=p1, p2=p2, readout=q))
        mean, std = _reference(c, p1, p2, q, k)
        print(f'{tag} p1={p1}: max|pred err|={np.abs(pred[:k] - mean - bias).max():.2e} '
              f'max|std err|={np.abs(sd[:k] - std).max():.2e}')
        _worst('oracle', n, pred[:k] - mean - bias, sd[:k] - std)
        np.testing.assert_allclose(pred[:k] - bias, mean, rtol=0, atol=ATOL, err_msg=f'{tag} p1={p1}')
        np.testing.assert_allclose(sd[:k], std, rtol=0, atol=ATOL, err_msg=f'{tag} p1={p1}')
        assert np.all(np.isfinite(pred)) and np.all(np.isfinite(sd)) and np.all(sd >= 0.0)


ORACLE_CASES = [(n, kind, trainable, readout) for n in (7, 8, 9) for kind in ('quanonet', 'heaqnn')
                for trainable in (True, False) for readout in (('Z', 'X', 'Y', 'diag') if n < 9 else ('Z', 'diag'))]


# ---- the tile index maps, without a GPU ----------------------------------------------------------------------------------------

def _tile_maps(n):
    """element -> (tile, local index) of stage A and stage B, as DESIGN.md 7t and hea_density_wide.hip state them"""
    i = np.arange(1 << (2 * n), dtype=np.int64)
    a = (i >> 12, i & 4095)
    hi = 2 * n - 8                                                       # the first bit of wires n-4 .. n-1
    b = ((i >> 4) & ((1 << (hi - 4)) - 1), (i & 15) | ((i >> hi) << 4))
    return a, b


def _pass_wires(J):
    """the two local wires Pass<6, J> loads: (t, c) = (J, J + 1 mod 6)"""
    return J, (J + 1) % 6


@pytest.mark.parametrize('n', [7, 8, 9])
def test_tile_maps(n):
    NE, tiles = 1 << (2 * n), 1 << (2 * (n - 6))
    i = np.arange(NE, dtype=np.int64)
    wires = {'A': (0, 1, 2, 3, 4, 5), 'B': (0, 1, n - 4, n - 3, n - 2, n - 1)}
    passes = {'A': range(0, 5), 'B': range(5, n)}
    for (tile, local), stage in zip(_tile_maps(n), 'AB'):
        assert tile.min() == 0 and tile.max() == tiles - 1 and local.min() == 0 and local.max() == 4095
        assert np.unique(tile * 4096 + local).size == NE                 # a bijection of 4^n
        for lw, w in enumerate(wires[stage]):                            # local wire lw is global wire w, both of its bits
            assert np.array_equal((local >> (2 * lw)) & 3, (i >> (2 * w)) & 3)
        rest = [w for w in range(n) if w not in wires[stage]]            # the tile index is the other wires' bits, in order
        want = sum(((i >> (2 * w)) & 3) << (2 * k) for k, w in enumerate(rest))
        assert np.array_equal(tile, want)
        # the inverse the kernel computes: element of (tile, local)
        back = tile << 12 | local if stage == 'A' else (local & 15) | tile << 4 | (local >> 4) << (2 * n - 8)
        assert np.array_equal(back, i)
        for j in passes[stage]:                                          # ring pass j = (target j, control j + 1 mod n)
            J = j if stage == 'A' else j - n + 6
            assert 0 <= J <= 5
            t, c = _pass_wires(J)
            assert (wires[stage][t], wires[stage][c]) == (j, (j + 1) % n)
    # stage B's one-qubit stages serve the wires stage A does not: local wire >= 12 - n is global wire >= 6
    assert [w for lw, w in enumerate(wires['B']) if lw >= 12 - n] == list(range(6, n))
    # every run of stage B in global memory is 16 contiguous elements
    tile, local = _tile_maps(n)[1]
    assert np.all(np.diff(i.reshape(-1, 16), axis=1) == 1) and np.all(np.diff(local.reshape(-1, 16), axis=1) == 1)
    assert np.all(tile.reshape(-1, 16) == tile.reshape(-1, 16)[:, :1])


def test_abi_checks_without_a_device():
    """symbols, version, the workspace size and everything the call refuses before it looks at a pointer"""
    from quanonet_amd import _lib
    lib = _lib.load()
    assert lib.qhea_version() >= 630 and _lib.MIN_LIB_VERSION >= 630
    for name in ('qhea_model_exact_noisy_wide_workspace_bytes', 'qhea_model_forward_noisy_exact_wide'):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    size, call = lib.qhea_model_exact_noisy_wide_workspace_bytes, lib.qhea_model_forward_noisy_exact_wide
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0)
    for n in (7, 8, 9):
        d = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
        tables = lib.qhea_model_noisy_wide_workspace_bytes(ctypes.byref(d), 100, ctypes.byref(ok))
        state = 100 * 4 ** n * 16
        assert state + 2 * 8 * 2 ** n < size(ctypes.byref(d), 100) < state + tables + 2 * 8 * 2 ** n + 512
        assert size(ctypes.byref(d), 3000) - size(ctypes.byref(d), 0) > 3000 * 4 ** n * 16      # past 2^32 bytes at n = 9
        assert size(ctypes.byref(d), -1) == 0
        assert call(ctypes.byref(d), 0, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == 0   # empty batch
        assert call(ctypes.byref(d), -1, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1
        assert call(ctypes.byref(d), 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1  # no pointers
        assert call(ctypes.byref(d), 10, None, None, None, None, None, None, None, None, 0, None) == -1   # no noise setting
        ignored = _lib.NoiseParams(0.01, 0.02, 0.03, -5, 0, 9)           # shots, trajectories and seed are ignored
        assert call(ctypes.byref(d), 0, None, None, None, None, ctypes.byref(ignored), None, None, None, 0, None) == 0
    assert size(None, 100) == 0
    for n in (2, 6, 10, 12):
        d = _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
        assert size(ctypes.byref(d), 100) == 0
        assert call(ctypes.byref(d), 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -2
        # a bad noise setting is reported before the qubit count
        assert call(ctypes.byref(d), 10, None, None, None, None, ctypes.byref(_lib.NoiseParams(2.0, 0, 0, 0, 1, 0)), None, None,
                    None, 0, None) == -1


# ---- 1. against the numpy density matrix ---------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n,kind,trainable,readout', ORACLE_CASES)
def test_against_the_oracle(dev, n, kind, trainable, readout):
    rows, k = (37, 3) if n < 9 else (5, 2)
    m = _model(kind, n, trainable, readout, seed=n).to(dev)
    ins = _inputs(kind, rows, dev, seed=rows)
    c, bias = _circuit(m, ins)
    _against_reference(m, ins, c, bias, NOISES, k, f'n={n} {kind} {trainable} {readout} {rows}', n)


@gpu
@pytest.mark.parametrize('kind,trainable,readout', [c[1:] for c in ORACLE_CASES if c[0] == 7])
def test_against_the_oracle_corner(dev, kind, trainable, readout):
    """p1 = p2 = readout = 1"""
    m = _model(kind, 7, trainable, readout, seed=7).to(dev)
    ins = _inputs(kind, 37, dev, seed=37)
    c, bias = _circuit(m, ins)
    _against_reference(m, ins, c, bias, ((1.0, 1.0, 1.0),), 3, f'n=7 {kind} {trainable} {readout} corner', 7)


# ---- 2. noiseless equals ideal -------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n', [7, 8, 9])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_noiseless_equals_ideal(dev, n, kind):
    from quanonet_amd.noise import NoiseModel
    for trainable in (True, False):
        for readout in ('Z', 'X', 'Y', 'diag'):
            m = _model(kind, n, trainable, readout, seed=n).to(dev)
            for rows in (1, 37, 300):
                ins = _inputs(kind, rows, dev, seed=rows)
                pred, sd = _wide(m, ins, NoiseModel(seed=5))
                ideal = _ideal(m, ins).cpu().numpy()
                tag = f'{trainable} {readout} {rows}'
                _worst('ideal', n, pred - ideal)
                np.testing.assert_allclose(pred, ideal, rtol=0, atol=ATOL, err_msg=tag)
                if rows <= 37:
                    c, bias = _circuit(m, ins)
                    psi = O.hea_state(c['n'], c['cfgs'], c['x'], c['w'])
                    NO._basis_change(psi, n, c['ham_pauli'])
                    prob = psi.real ** 2 + psi.imag ** 2
                    kk = np.arange(1 << n)
                    hv = c['ham_diag'] if c['ham_diag'] is not None else \
                        c['offset'] + c['coeff'] * (n - 2.0 * sum((kk >> i) & 1 for i in range(n)))
                    mean = prob @ hv
                    std = np.sqrt(np.maximum(prob @ (hv * hv) - mean ** 2, 0.0))
                    _worst('ideal', n, pred - mean - bias, sd - std)
                    np.testing.assert_allclose(pred, mean + bias, rtol=0, atol=ATOL, err_msg=tag)
                    np.testing.assert_allclose(sd, std, rtol=0, atol=ATOL, err_msg=tag)


# ---- 3. stage edges ------------------------------------------------------------------------------------------------------------

def _edge_model(shape, n, readout):
    kw = dict(if_trainable_freq=True, scale_coeff=0.7, ham_bound=(-2.0, 3.0), ham_pauli=readout)
    if shape == 'heaqnn-ld0':
        return 'heaqnn', H.heaqnn(n, 4, (2, 0), 3, **kw)                 # encoding blocks only
    if shape == 'quanonet-ld0':
        return 'quanonet', H.quanonet(n, 3, 2, (2, 0, 1, 2), 3, **kw)    # a sub-layer stage first, one-qubit stages behind it
    if shape == 'ld0-first':
        return 'quanonet', H.quanonet(n, 3, 2, (1, 1, 2, 0), 3, **kw)    # a one-qubit stage is the first of the circuit
    return 'heaqnn', H.heaqnn(n, 4, (1, 1), 3, **kw)                     # one sub-layer


@gpu
@pytest.mark.parametrize('n', [7, 9])
@pytest.mark.parametrize('shape', ['heaqnn-ld0', 'quanonet-ld0', 'ld0-first', 'one-sublayer'])
def test_stage_edges(dev, n, shape):
    for readout in ('Z', 'Y'):
        kind, m = _edge_model(shape, n, readout)
        m = m.to(dev)
        ins = _inputs(kind, 2, dev, seed=n)
        c, bias = _circuit(m, ins)
        _against_reference(m, ins, c, bias, NOISES[:1], 2, f'n={n} {shape} {readout}', n)


@gpu
@pytest.mark.parametrize('n,rows', [(7, 1), (7, 3), (8, 1), (9, 1)])
def test_small_batches(dev, n, rows):
    """batch 1, and a batch of 3 rows"""
    m = _model('quanonet', n, True, 'X', seed=n + 1).to(dev)
    ins = _inputs('quanonet', rows, dev, seed=n)
    c, bias = _circuit(m, ins)
    _against_reference(m, ins, c, bias, NOISES[:1], min(rows, 2 if n == 9 else 3), f'n={n} rows={rows}', n)


# ---- 4. determinism and chunking -----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n,kind,rows', [(7, 'quanonet', 1000), (9, 'heaqnn', 40)])
def test_deterministic_and_chunk_independent(dev, n, kind, rows):
    from quanonet_amd.noise import NoiseModel
    m = _model(kind, n, True, 'Z', seed=2).to(dev)
    ins = _inputs(kind, rows, dev, seed=3)
    nz = NoiseModel(p1=0.02, p2=0.05, readout=0.03)
    a, sa = _wide(m, ins, nz)
    b, sb = _wide(m, ins, nz)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    for chunk in (7, 64, rows):
        c, sc = _wide(m, ins, nz, chunk_rows=chunk)
        assert np.array_equal(a, c) and np.array_equal(sa, sc), chunk
    lo, hi = rows * 3 // 10, rows * 3 // 10 + min(37, rows // 4)
    part = tuple(t[lo:hi] for t in ins)                                  # a slice of the rows is the same rows of the whole call
    p, s = _wide(m, part, nz)
    assert np.array_equal(p, a[lo:hi]) and np.array_equal(s, sa[lo:hi])
    d, sdd = _wide(m, ins, NoiseModel(p1=0.02, p2=0.05, readout=0.03, shots=17, trajectories=3, seed=99))
    assert np.array_equal(a, d) and np.array_equal(sa, sdd)              # shots, trajectories and seed are ignored


@gpu
def test_small_n_is_exact_noisy_predict(dev):
    from quanonet_amd.noise import DeviceNoise, NoiseModel, exact_noisy_predict, wide_exact_noisy_predict
    m = _model('quanonet', 5, True, 'Z', seed=2).to(dev)
    ins = _inputs('quanonet', 100, dev, seed=3)
    nz = NoiseModel(p1=0.02, p2=0.05, readout=0.03)
    for noise in (nz, DeviceNoise.uniform(nz)):
        for kw in ({}, {'chunk_rows': 33}):
            p, s = exact_noisy_predict(m, ins, noise)
            wp, ws = wide_exact_noisy_predict(m, ins, noise, **kw)
            assert torch.equal(p, wp) and torch.equal(s, ws)


def test_default_chunk():
    from quanonet_amd.noise import WIDE_EXACT_STATE_BYTES
    """the largest row count whose density matrices stay within 256 MiB: the fastest of the sweep at n = 8 and 9 (64 MiB,
    256 MiB, 1 GiB; profiles/r37_exact_noisy_wide_rate.json), ahead of 1 GiB by 16 % against a run-to-run spread under 1 %"""
    assert WIDE_EXACT_STATE_BYTES == 1 << 28
    assert [WIDE_EXACT_STATE_BYTES >> (2 * n + 4) for n in (7, 8, 9)] == [1024, 256, 64]


# ---- 5. errors launch nothing --------------------------------------------------------------------------------------------------

@gpu
def test_errors_launch_nothing(dev):
    from quanonet_amd import _lib
    m = _model('quanonet', 7, True, 'Z').to(dev)
    ins = _inputs('quanonet', 10, dev)
    desc, params = m.fused_desc(), H.flat(m)
    out = torch.full((10,), 123.0, dtype=torch.float64, device=dev)
    sd = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0)
    for bad in (_lib.NoiseParams(-0.01, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.5, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
                _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0)):
        with pytest.raises(_lib.QheaError):
            _lib.model_forward_noisy_exact_wide(desc, ins[0], ins[1], params, bad, out=out, shot_std=sd)
    for n in (6, 10):
        mo = _model('heaqnn', n, True, 'Z').to(dev)
        io = _inputs('heaqnn', 10, dev)
        assert _lib.load().qhea_model_exact_noisy_wide_workspace_bytes(ctypes.byref(mo.fused_desc()), 10) == 0
        with pytest.raises(_lib.Unsupported):
            _lib.model_forward_noisy_exact_wide(mo.fused_desc(), io[0], None, H.flat(mo), ok, out=out, shot_std=sd)
    # a short workspace, through the C entry
    lib = _lib.load()
    need = lib.qhea_model_exact_noisy_wide_workspace_bytes(ctypes.byref(desc), 10)
    assert need >= 10 * (4 ** 7) * 16
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args = [ctypes.byref(desc), 10, _lib._ptr(ins[0]), _lib._ptr(ins[1]), _lib._ptr(params), None, ctypes.byref(ok),
            _lib._ptr(out), _lib._ptr(sd), _lib._ptr(ws)]
    with torch.cuda.device(dev):
        assert lib.qhea_model_forward_noisy_exact_wide(*args, need - 1, _lib._stream(dev)) == -3
        assert lib.qhea_model_forward_noisy_exact_wide(*args[:-1], None, need, _lib._stream(dev)) == -3
    torch.cuda.synchronize()
    assert torch.all(out == 123.0) and torch.all(sd == 456.0)
    # shot_std is optional
    pred, none = _lib.model_forward_noisy_exact_wide(desc, ins[0], ins[1], params, ok)
    both, _ = _lib.model_forward_noisy_exact_wide(desc, ins[0], ins[1], params, ok, shot_std=sd)
    torch.cuda.synchronize()
    assert none is None and torch.equal(pred, both) and torch.all(sd != 456.0)


@gpu
@pytest.mark.parametrize('n', [7, 8, 9])
def test_grid_guard(dev, n):
    """A stage has one workgroup per (row, tile), rows x 4^(n-6) of them in gridDim.x: the first batch that passes INT_MAX is
    refused as a bad argument, before the workspace is looked at.  The workspace here holds one row, so without the guard the
    call would answer -3: nothing is launched either way, and the largest batch the guard admits does answer -3."""
    from quanonet_amd import _lib
    lib = _lib.load()
    m = _model('heaqnn', n, True, 'Z').to(dev)
    ins = _inputs('heaqnn', 2, dev)
    desc, params = m.fused_desc(), H.flat(m)
    out = torch.full((2,), 123.0, dtype=torch.float64, device=dev)
    sd = torch.full((2,), 456.0, dtype=torch.float64, device=dev)
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0)
    need = lib.qhea_model_exact_noisy_wide_workspace_bytes(ctypes.byref(desc), 1)
    assert need >= (4 ** n) * 16
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    limit = (2 ** 31 - 1) >> (2 * (n - 6))

    def call(batch):
        return lib.qhea_model_forward_noisy_exact_wide(ctypes.byref(desc), batch, _lib._ptr(ins[0]), None, _lib._ptr(params), None,
                                                       ctypes.byref(ok), _lib._ptr(out), _lib._ptr(sd), _lib._ptr(ws), need,
                                                       _lib._stream(dev))
    with torch.cuda.device(dev):
        assert call(limit + 1) == -1
        assert call(limit) == -3
    torch.cuda.synchronize()
    _lib.check_status(dev)
    assert torch.all(out == 123.0) and torch.all(sd == 456.0)


@gpu
def test_python_refusals(dev):
    from quanonet_amd.noise import DeviceNoise, NoiseModel, exact_noisy_predict, wide_exact_noisy_predict
    from quanonet_amd import _lib
    nz = NoiseModel(p1=0.01, p2=0.02, readout=0.01)
    m8 = _model('heaqnn', 8, True, 'Z').to(dev)
    ins = _inputs('heaqnn', 4, dev)
    with pytest.raises(ValueError, match='exact_noisy_predict.*device_noisy_predict'):
        wide_exact_noisy_predict(m8, ins, DeviceNoise.uniform(nz))
    with pytest.raises(ValueError, match='noisy_predict'):
        wide_exact_noisy_predict(_model('heaqnn', 10, True, 'Z').to(dev), ins, nz)
    with pytest.raises(_lib.Unsupported):                                # the n <= 6 call keeps its range
        exact_noisy_predict(m8, ins, nz)


# ---- 6. graph capture and launch count -----------------------------------------------------------------------------------------

def _is_kernel(name, ident, n=None):
    """whether a mangled kernel name is `ident` of this unit's unnamed namespace (`_GLOBAL__N_1`, whose last character is a
    digit: helpers.mangled_is reads it as part of the length prefix), with first template argument n where given"""
    return f'_GLOBAL__N_1{len(ident)}{ident}' + ('' if n is None else f'ILi{n}E') in name


def test_is_kernel():
    ring = '_ZN4qhea12_GLOBAL__N_124density_wide_ring_kernelILi7ELi1EEEvNS0_8DensArgsEP15HIP_vector_typeIdLj2EEiiii'
    assert _is_kernel(ring, 'density_wide_ring_kernel') and _is_kernel(ring, 'density_wide_ring_kernel', 7)
    assert not _is_kernel(ring, 'density_wide_ring_kernel', 9) and not _is_kernel(ring, 'density_wide_wires_kernel')
    assert not _is_kernel(ring, 'wide_ring_kernel') and not _is_kernel(ring, 'density_wide_ring')


@gpu
@pytest.mark.parametrize('n', [7, 9])
@pytest.mark.parametrize('readout', ['Z', 'X'])
def test_graph_capturable_launch_count(dev, n, readout):
    from quanonet_amd import _lib
    from quanonet_amd.noise import NoiseModel
    rows = 5
    nz = NoiseModel(p1=0.01, p2=0.02).params()
    kw = dict(if_trainable_freq=True, scale_coeff=0.7, ham_pauli=readout)
    for m, kind, sublayers, ld0 in ((_model('quanonet', n, True, readout), 'quanonet', 4, 0),
                                    (H.quanonet(n, 3, 2, (2, 0, 1, 2), 3, **kw), 'quanonet', 2, 2)):
        m = m.to(dev)
        ins = _inputs(kind, rows, dev)
        desc, params = m.fused_desc(), H.flat(m)
        out = torch.empty(rows, dtype=torch.float64, device=dev)
        sd = torch.empty(rows, dtype=torch.float64, device=dev)
        call = lambda: _lib.model_forward_noisy_exact_wide(desc, ins[0], ins[1], params, nz, out=out, shot_std=sd)
        call()                                                           # sizes the workspace outside the capture
        torch.cuda.synchronize()
        eager = (out.clone(), sd.clone())
        launches = H.kernel_launches(dev, call)
        stages = [k for k in launches if _is_kernel(k[0], 'density_wide_ring_kernel', n) or
                  _is_kernel(k[0], 'density_wide_wires_kernel', n)]
        others = [k[0] for k in launches if k not in stages]
        assert len(stages) == 2 * sublayers + 2 * ld0 + (2 if readout == 'X' else 0), [k[0] for k in launches]
        assert sum(_is_kernel(k[0], 'density_wide_ring_kernel', n) for k in stages) == 2 * sublayers
        for k in stages:
            assert k[1] == (rows * 4 ** (n - 6), 1, 1) and k[2] == (256, 1, 1), k
        assert len(others) == 3 and 'prep_model_kernel' in others[0] and 'density_wide_values_kernel' in others[1] and \
            _is_kernel(others[2], 'density_wide_readout_kernel', n), others
        assert launches[-1][0] == others[2] and [k[0] for k in launches[:2]] == others[:2]
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(sd, eager[1])


# ---- 7. the wide trajectory kernels against the exact value --------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n', [7, 8, 9])
@pytest.mark.parametrize('shots', [0, 20000])
def test_trajectory_kernel_against_exact(dev, n, shots):
    """
    test_exact_noisy.test_trajectory_kernel_against_exact at n = 7..9: the wave-resident trajectory kernels of
    hea_noise_wide.hip against the exact value.  The bound is a condition on a correct kernel, not a measurement: the
    estimator is unbiased, the seeds are fixed here, and over the 96 compared values a correct kernel leaves 5 stderr with
    probability about 5e-5.
    The n = 7 stream was replayed on the CPU first (noise_oracle.replay_values, rows 0 and 1, against
    density_reference.exact_moments): seed 1007, largest |z| 0.33 in expectation mode and 0.51 in shot mode, shot-mode
    stderr sqrt(S) / shot_std within [0.999, 1.001].
    """
    from quanonet_amd.noise import NoiseModel
    m = _model('heaqnn', n, True, 'Z', seed=n + 20).to(dev)
    ins = _inputs('heaqnn', 16, dev, seed=n)
    nz = NoiseModel(p1=0.03, p2=0.08, readout=0.04, shots=shots, trajectories=20000, seed=1000 + n)
    pred, se = _noisy(m, ins, nz)
    exact, sd = _wide(m, ins, nz)
    assert np.all(se > 0)
    print(f'n={n} shots={shots}: z={(pred - exact) / se}')
    assert np.all(np.abs(pred - exact) < 5 * se), (pred - exact) / se
    if shots:
        print(f'stderr sqrt(S) / shot_std = {se * np.sqrt(shots) / sd}')
        assert np.all(np.abs(se * np.sqrt(shots) / sd - 1.0) < 0.1), se * np.sqrt(shots) / sd


# ---- 8. solvers ----------------------------------------------------------------------------------------------------------------

@gpu
def test_solver_evaluate_noisy_wide(dev, tmp_path):
    from quanonet_amd import _lib
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import NoiseModel, Sampling, wide_exact_noisy_predict
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
    nz = NoiseModel(p1=0.01, p2=0.02, readout=0.01, shots=200, seed=9)
    y_true = torch.tensor(data['test_output'], device=dev)
    res = s.evaluate_noisy(nz, exact='wide')
    assert set(os.listdir(s.out_dir)) == files
    pred, sd = wide_exact_noisy_predict(s.model, s.test_input, nz)
    for k, v in regression_metrics(pred, y_true).items():
        assert res[k] == v, k
    assert res['exact'] is True and res['mean_shot_std'] == float(sd.mean().item()) and res['noise'] == nz.asdict()
    assert 'mean_stderr' not in res
    res2 = s.evaluate_noisy(nz, out_name='wide_metric.json', exact='wide')
    assert set(os.listdir(s.out_dir)) == files | {'wide_metric.json'}
    with open(os.path.join(s.out_dir, 'wide_metric.json')) as f:
        assert json.load(f) == json.loads(json.dumps(res2))
    assert (open(mpath).read(), os.stat(mpath).st_mtime_ns) == before
    with pytest.raises(_lib.Unsupported):                                # exact=True keeps its range
        s.evaluate_noisy(nz, exact=True)
    with pytest.raises(ValueError, match="'tiled'"):
        s.evaluate_noisy(nz, exact='tiled')
    with pytest.raises(ValueError, match='sampling='):
        s.evaluate_noisy(nz, exact='wide', sampling=Sampling(seed=1))
    assert (open(mpath).read(), os.stat(mpath).st_mtime_ns) == before and set(os.listdir(s.out_dir)) == files | {'wide_metric.json'}
    ens = EnsembleSolver([dict(cfg, seed=k, run_id=f'm{k}', prefix=str(tmp_path / 'ens')) for k in (0, 1)], data, device=dev,
                         log=quiet)
    ens.train()
    outs = ens.evaluate_noisy(nz, exact='wide')
    assert len(outs) == 2
    for mem, o in zip(ens.members, outs):
        p, _ = wide_exact_noisy_predict(mem.model, mem.test_input, nz)
        assert o['exact'] is True and o['MSE'] == regression_metrics(p, y_true)['MSE']
        assert not os.path.exists(os.path.join(mem.out_dir, 'metric.json'))
