"""
CPU checks of the workgroup-resident device-noise trajectory call (qhea_model_forward_noisy_device_wide, n = 10..12): the design's
proof -- the kernel's formulation restated in numpy (tests/device_traj_wide_reference.py: pre-ring labels, a frame the jumps
update, at most three stored bits per site, unnormalised state) against the literal gate-by-gate replay of
tests/device_traj_reference.py on the same random stream -- and the C ABI's symbols, argument checks and workspace sizes
(nothing is launched, no GPU needed).

Tolerance of the proof.  Both sides are fp64 and see the same few hundred operations per amplitude in a different association
(normalise at every site against once at the end): 1e-12 on values of order one, the tolerance of tests/test_device_traj.py.  A
decision differs only where u lies within a few ulps of an edge: about 1e4 decisions per case, a chance below 1e-10 over the set.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import device_traj_reference as TR
from tests import device_traj_wide_reference as WR
from tests.conftest import ROOT
from tests.test_device_noise_abi import BAD, _random_noise, _record
from tests.test_device_traj import _as_dict, _strong
from tests.test_noisy_forward import _circuit, _inputs, _model


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_site_masks():
    """the mask table against the ring applied CNOT by CNOT: after slots 0..j the logical bit of the site's wire is the parity
    of the stored bits in the mask"""
    for n in (3, 4, 5, 10, 11, 12):
        k = np.arange(1 << n)
        logical = k.copy()
        for j in range(n):
            c, t = (j + 1) % n, j
            logical = logical ^ (((logical >> c) & 1) << t)
            for kind in (TR.TGT, TR.CTL):
                wire, mask = WR.site_mask(n, kind, j)
                assert wire == (t if kind == TR.TGT else c) and bin(mask).count('1') <= 3
                assert np.array_equal((logical >> wire) & 1, WR._parity(k & mask)), (n, kind, j)
        assert np.array_equal(logical, WR.ring_map(n))


@pytest.mark.parametrize('n,kind,readout,idle', list(itertools.product((3, 4, 10), ('quanonet', 'heaqnn'), ('Z', 'Y', 'diag'),
                                                                        (True, False))))
def test_formulation_equals_the_replay(n, kind, readout, idle):
    rows, T = (5, 24) if n < 10 else (2, 4)
    m = _model(kind, n, True, readout, seed=3)
    ins = _inputs(kind, rows, 'cpu', seed=rows + n)
    c, _ = _circuit(m, ins)
    nz = _as_dict(_strong(n, idle), n)
    args = (c['n'], c['cfgs'], c['x'], c['w'], nz)
    kw = dict(offset=c['offset'], coeff=c['coeff'], ham_diag=c['ham_diag'], ham_pauli=c['ham_pauli'], row0=11)
    for shots in (0, T):
        want_counts, got_counts = {}, {}
        want = TR.replay_values(*args, shots, T, 77, counts=want_counts, **kw)
        got = WR.formulation_values(*args, shots, T, 77, counts=got_counts, **kw)
        print(f'n={n} {kind} {readout} idle={idle} shots={shots}: max|diff|={np.abs(got - want).max():.2e} events={want_counts}')
        assert got_counts == want_counts
        assert min(want_counts.values()) >= 1, want_counts
        if shots:
            assert np.array_equal(got, want)
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 570 and _lib.MIN_LIB_VERSION >= 570
    for name in ('qhea_model_noisy_device_wide_workspace_bytes', 'qhea_model_forward_noisy_device_wide'):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert callable(_lib.model_forward_noisy_device_wide) and callable(_lib.model_noisy_device_wide_workspace_bytes)


def test_abi_argument_checks_without_gpu(lib):
    from quanonet_amd import _lib
    call, ws_bytes = lib.qhea_model_forward_noisy_device_wide, lib.qhea_model_noisy_device_wide_workspace_bytes
    sp = _lib.SamplingParams(0, 3, 1)

    def desc(n, model=_lib.MODEL_HEAQNN):
        if model == _lib.MODEL_QUANONET:
            return _lib.make_model_desc(model, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
        return _lib.make_model_desc(model, n, (2, 1), 4, 0, True, 0.1, 0.0, 1.0)

    def run(d, rec, samp, batch=4, row0=0):
        return call(ctypes.byref(d), row0, batch, None, None, None, None, None if rec is None else ctypes.byref(rec),
                    None if samp is None else ctypes.byref(samp), None, None, None, 0, None)

    bad_sampling = [_lib.SamplingParams(-1, 1, 0), _lib.SamplingParams(0, 0, 0), _lib.SamplingParams(0, -5, 0),
                    _lib.SamplingParams(1 << 32, 1, 0), _lib.SamplingParams(0, 1 << 32, 0)]
    for n in (10, 11, 12):
        d, ok = desc(n), _record(n)
        assert run(d, ok, sp, batch=0) == 0                              # empty batch
        assert run(d, ok, sp, batch=-1) == -1 and run(d, ok, sp, row0=-1) == -1
        assert run(d, ok, sp) == -1                                      # NULL arrays
        assert run(d, None, sp) == -1 and run(d, ok, None) == -1
        assert run(d, _record(n - 1), sp, batch=0) == -1                 # n_wires != n
        assert ws_bytes(ctypes.byref(d), 8, ctypes.byref(sp)) > 0
    d10, d9 = desc(10), desc(9)
    # the header's order: the device record and the sampling record (-1), then the qubit range (-2)
    for over in BAD:
        assert run(d10, _record(10, **over), sp, batch=0) == -1, over
        assert run(d9, _record(9, **over), sp, batch=0) == -1, over
    for bad in bad_sampling:
        assert run(d10, _record(10), bad, batch=0) == -1 and run(d9, _record(9), bad, batch=0) == -1
        assert ws_bytes(ctypes.byref(d10), 8, ctypes.byref(bad)) == 0
    for n in (2, 5, 9):
        dn_ = desc(n, _lib.MODEL_QUANONET)
        assert run(dn_, _record(n), sp) == -2 and run(dn_, _record(n), sp, batch=0) == -2
        assert ws_bytes(ctypes.byref(dn_), 8, ctypes.byref(sp)) == 0
    assert run(d10, _record(10), _lib.SamplingParams((1 << 32) - 1, 0, 0), batch=0) == 0
    # workspace sizes
    assert ws_bytes(ctypes.byref(d10), 8, None) == 0 and ws_bytes(ctypes.byref(d10), -1, ctypes.byref(sp)) == 0
    bad_desc = _lib.make_model_desc(_lib.MODEL_QUANONET, 1, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    assert ws_bytes(ctypes.byref(bad_desc), 8, ctypes.byref(sp)) == 0
    d12 = desc(12, _lib.MODEL_QUANONET)
    small = ws_bytes(ctypes.byref(d12), 8, ctypes.byref(sp))
    assert ws_bytes(ctypes.byref(d12), 8, ctypes.byref(_lib.SamplingParams(0, 1000, 0))) > small > 0
    assert _lib.model_noisy_device_wide_workspace_bytes(d12, 8, sp) == small
    # the old call keeps its range
    assert lib.qhea_model_noisy_device_workspace_bytes(ctypes.byref(d10), 8, ctypes.byref(sp)) == 0
    assert lib.qhea_model_noisy_device_workspace_bytes(ctypes.byref(d9), 8, ctypes.byref(sp)) > 0


@pytest.mark.parametrize('idle', [True, False])
def test_jump_tables_at_12_wires(lib, idle):
    n = 12
    nz = _random_noise(n, seed=99 + idle, idle=idle)
    jump = nz.jump_tables(n)
    assert jump.shape == (4, n, 2)
    np.testing.assert_allclose(jump, TR.jump_pairs(n, _as_dict(nz, n)), rtol=0, atol=1e-15)


def test_python_surface_without_gpu():
    from quanonet_amd import noise as N
    assert '2..12' in N.device_noisy_predict.__doc__
