"""
CPU checks of the sampled-trajectory gradient at n = 10..12 (qhea_model_loss_grad_noisy_lds / qhea_model_train_steps_noisy_lds):
the numpy reference tests/noisy_traj_grad_reference.py at those sizes against the ideal oracle and against central differences
of the replay (the bounds of the n = 7 tests), the C ABI's symbols and argument checks (nothing is launched, no GPU needed), and
the index and sign arithmetic of the framed LDS store and its mirror (hea_lds.hpp) on the host.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import hea_oracle as O
from tests import noisy_traj_grad_reference as TG
from tests.test_noisy_traj_grad_reference import noise_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
NEW = ('qhea_model_noisy_lds_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_lds', 'qhea_model_train_steps_noisy_lds')


def _point(n, seed):
    """blocks [(n, 1), (n, 2)], 2 rows: (cfgs, x[2, 2n], w[3, 3, n])"""
    rng = np.random.default_rng(seed)
    return [(n, 1), (n, 2)], rng.uniform(-1.5, 1.5, (2, 2 * n)), rng.uniform(-np.pi, np.pi, (3, 3, n))


@pytest.mark.parametrize('n', [10, 11, 12])
def test_noiseless_reference_is_the_ideal_oracle(n):
    cfgs, x, w = _point(n, n)
    v, gx, gw = TG.traj_grad(n, cfgs, x, w, noise_model((0.0, 0.0, 0.0)), offset=0.3, coeff=0.7, row0=3_000_000_000)
    ref = O.hea_forward(n, cfgs, x, w, 0.3, 0.7)
    np.testing.assert_allclose(v, ref, rtol=0, atol=1e-12)
    for b in range(2):                                        # the oracle's backward sums over the rows: one row at a time
        g = np.zeros(2)
        g[b] = 1.0
        _, rx, rw = O.hea_backward(n, cfgs, x, w, g, 0.3, 0.7)
        np.testing.assert_allclose(gx[b], np.asarray(rx)[b], rtol=0, atol=1e-12)
        np.testing.assert_allclose(gw[b], rw, rtol=0, atol=1e-12)


@pytest.mark.parametrize('n', [10, 11, 12])
def test_adjoint_and_central_difference_forms_agree(n):
    cfgs, x, w = _point(n, 20 + n)
    nz = noise_model((0.05, 0.1, 0.05), T=3, seed=9)
    adj = TG.traj_grad(n, cfgs, x, w, nz, coeff=0.7, row0=3_000_000_000)
    cd = TG.traj_grad_shift(n, cfgs, x, w, nz, coeff=0.7, row0=3_000_000_000)
    for a, c in zip(adj, cd):
        np.testing.assert_allclose(a, c, rtol=0, atol=1e-12)
    assert np.abs(adj[2]).max() > 1e-3 and np.abs(adj[1]).max() > 1e-3


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 590 and _lib.MIN_LIB_VERSION >= 590
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    for f in (_lib.model_loss_grad_noisy_lds, _lib.model_train_steps_noisy_lds, _lib.model_noisy_lds_grad_workspace_bytes):
        assert callable(f)
    from quanonet_amd.noise import sampled_noisy_loss_and_grad
    assert callable(sampled_noisy_loss_and_grad)


def _loss_grad(lib, d, batch, nz, name='qhea_model_loss_grad_noisy_lds', row0=0):
    """the call with every array NULL: what the checks in front of the pointers return"""
    return getattr(lib, name)(None if d is None else ctypes.byref(d), row0, batch, None, None, None, None, None,
                              None if nz is None else ctypes.byref(nz), 1.0, None, None, None, 0, None)


def _train_steps(lib, d, n_steps, nz, name='qhea_model_train_steps_noisy_lds', first_step=1):
    return getattr(lib, name)(None if d is None else ctypes.byref(d), n_steps, None, None, None, None, None, None,
                              None if nz is None else ctypes.byref(nz), None, None, 0, None, None, first_step, 1e-3, 0.9, 0.999,
                              1e-8, 0.0, None, 0, None)


def test_abi_argument_checks_without_gpu(lib):
    from quanonet_amd import _lib
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, 10, (2, 1, 2, 2), 3, 2, True, 0.1, 0.0, 1.0)
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 40, 5)
    size = lambda dd, b, nz: lib.qhea_model_noisy_lds_grad_workspace_bytes(None if dd is None else ctypes.byref(dd), b,
                                                                           None if nz is None else ctypes.byref(nz))
    # (E + 3 n blk) doubles per (row, tile of 2) and per row: E = 40, blk = 6, T = 40 -> 20 tiles
    width, tiles = 40 + 3 * 10 * 6, 20
    assert size(d, 100, ok) >= 8 * 100 * (tiles + 1) * width > 0
    assert size(d, 0, ok) <= size(d, 1, ok) <= size(d, 99, ok) <= size(d, 100, ok) <= size(d, 101, ok)
    assert size(d, -1, ok) == 0 and size(None, 100, ok) == 0 and size(d, 100, None) == 0
    assert size(d, 100, _lib.NoiseParams(0.01, 0.02, 0.03, 10, 40, 5)) == 0              # shot mode has no gradient
    assert size(d, 100, _lib.NoiseParams(0.01, 0.02, 0.03, 0, 0, 5)) == 0                # trajectories < 1
    for bad in (_lib.NoiseParams(-0.1, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.01, 0, 0, 1, 0),
                _lib.NoiseParams(0, 0, float('nan'), 0, 1, 0)):
        assert size(d, 100, bad) == 0
    small = {n: _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (2, 1), 3, 0, False, 0.1, 0.0, 1.0) for n in (2, 6, 7, 9)}
    d12 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 12, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    assert all(size(dn, 100, ok) == 0 for dn in small.values()) and size(d12, 100, ok) > 0
    d9 = small[9]
    bad_desc = _lib.make_model_desc(_lib.MODEL_QUANONET, 10, (2, 1, 2, 2), 3, 2, True, 0.1, 0.0, 1.0)
    bad_desc.n_qubits = 0
    bads = (_lib.NoiseParams(-0.1, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0), _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0),
            _lib.NoiseParams(0.01, 0.02, 0.03, 0, 0, 0),                                  # trajectories < 1
            _lib.NoiseParams(0.01, 0.02, 0.03, 7, 40, 0))                                 # shots
    for call in (_loss_grad, _train_steps):
        # the header's order: the descriptor, the noise setting, the qubit count, then the rest
        assert call(lib, bad_desc, 10, ok) == -1 and call(lib, None, 10, ok) == -1
        for bad in bads:
            assert call(lib, d, 10, bad) == -1
            assert call(lib, d9, 10, bad) == -1                                   # the noise setting is reported before the qubit count
        assert call(lib, d, 10, None) == -1
        assert call(lib, d9, 10, ok) == -2 and call(lib, small[6], 10, ok) == -2
        assert call(lib, d9, 0, ok) == -2                                         # the qubit range comes before the empty batch
        assert call(lib, d, -1, ok) == -1
        assert call(lib, d, 0, ok) == 0                                           # empty batch / no steps
        assert call(lib, d, 10, ok) == -1 and call(lib, d12, 10, ok) == -1        # valid up to the NULL arrays
    assert _loss_grad(lib, d, 10, ok, row0=-1) == -1
    assert _loss_grad(lib, d9, -1, ok) == -2                                      # the qubit range comes before a negative batch
    assert _train_steps(lib, d, 3, ok, first_step=0) == -1
    assert _train_steps(lib, d9, 3, ok, first_step=0) == -1                       # first_step opens the steps call, as in the _wide pair
    # the _wide pair keeps its answers at n = 10
    assert _loss_grad(lib, d, 10, ok, name='qhea_model_loss_grad_noisy_wide') == -2
    assert _train_steps(lib, d, 3, ok, name='qhea_model_train_steps_noisy_wide') == -2
    assert lib.qhea_model_noisy_wide_grad_workspace_bytes(ctypes.byref(d), 100, ctypes.byref(ok)) == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_framed_store_and_its_mirror_on_the_host(tmp_path):
    """tests/native/frame_mirror_check.cpp: for n = 10..12, both pass widths, every pass base, both RING settings, all k and 300
    (x, z) pairs -- the scatter stays in bounds and is one-to-one, realises the frame, and the gather undoes it"""
    exe = str(tmp_path / 'frame_mirror_check')
    src = os.path.join(ROOT, 'tests', 'native', 'frame_mirror_check.cpp')
    r = subprocess.run([HIPCC, '-O2', '-std=c++17', '-x', 'hip', '--offload-arch=gfx950', '-I', os.path.join(ROOT, 'include'),
                        '-I', os.path.join(ROOT, 'quanonet_amd', 'csrc'), src, '-o', exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe, '300'], stdout=subprocess.PIPE, text=True, timeout=300)
    words = out.stdout.split()
    assert out.returncode == 0 and words[-2:] == ['failed', '0'], out.stdout[-2000:]
    # 6 layouts (n = 10..12 x LG = 3, 4), 4 or 3 passes each, 2 RING settings, 300 pairs
    assert int(words[-3]) == (3 * 4 + 3 * 3) * 2 * 300
