"""
CPU checks of the exact noisy forward (qhea_model_forward_noisy_exact): the symbols and the C ABI's argument checks (nothing is
launched, no GPU needed), and the n-general density-matrix reference of tests/density_reference.py against the oracle's
exact_values at n = 2..5, all four read-outs.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import hea_oracle as O
from tests import density_reference as DR
from tests import noise_oracle as NO
from tests.conftest import ROOT


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 510
    for name in ('qhea_model_exact_noisy_workspace_bytes', 'qhea_model_forward_noisy_exact'):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert callable(_lib.model_forward_noisy_exact)
    from quanonet_amd.noise import exact_noisy_predict
    assert callable(exact_noisy_predict)


def test_abi_argument_checks_without_gpu(lib):
    from quanonet_amd import _lib
    call = lib.qhea_model_forward_noisy_exact
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, 5, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0)
    # header + gate table + (cos, sin) of 100 rows x 20 encoding columns
    assert lib.qhea_model_exact_noisy_workspace_bytes(ctypes.byref(d), 100) > 100 * 20 * 16
    assert lib.qhea_model_exact_noisy_workspace_bytes(ctypes.byref(d), -1) == 0
    bad_desc = _lib.make_model_desc(_lib.MODEL_QUANONET, 5, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    bad_desc.n_qubits = 0
    assert lib.qhea_model_exact_noisy_workspace_bytes(ctypes.byref(bad_desc), 100) == 0
    assert lib.qhea_model_exact_noisy_workspace_bytes(None, 100) == 0
    assert call(ctypes.byref(bad_desc), 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1
    assert call(ctypes.byref(d), 0, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == 0   # empty batch
    for bad in (_lib.NoiseParams(-0.1, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.01, 0, 0, 1, 0),
                _lib.NoiseParams(0, 0, float('nan'), 0, 1, 0), _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0),
                _lib.NoiseParams(0, 0, 2.0, 0, 1, 0)):
        assert call(ctypes.byref(d), 10, None, None, None, None, ctypes.byref(bad), None, None, None, 0, None) == -1
    assert call(ctypes.byref(d), 10, None, None, None, None, None, None, None, None, 0, None) == -1     # no noise setting
    # shots, trajectories and seed are ignored: values the trajectory call rejects pass the checks (and reach the NULL pointers)
    ignored = _lib.NoiseParams(0.01, 0.02, 0.03, -5, 0, 9)
    assert call(ctypes.byref(d), 0, None, None, None, None, ctypes.byref(ignored), None, None, None, 0, None) == 0
    assert call(ctypes.byref(d), -1, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    assert call(ctypes.byref(d7), 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -2
    # a bad noise setting is reported before the qubit count
    assert call(ctypes.byref(d7), 10, None, None, None, None, ctypes.byref(_lib.NoiseParams(2.0, 0, 0, 0, 1, 0)), None, None,
                None, 0, None) == -1
    # X / Y read-outs do not combine with ham_diag (as in every other call)
    dx = _lib.make_model_desc(_lib.MODEL_QUANONET, 3, (1, 1, 1, 1), 4, 1, True, 0.1, 0.0, 1.0)
    dx.ham_pauli = 1
    assert call(ctypes.byref(dx), 10, None, None, None, ctypes.c_void_p(256), ctypes.byref(ok), None, None, None, 0,
                None) == -1


def _circuit(n, rows, ld=1, blocks=2, seed=0):
    rng = np.random.default_rng(seed)
    cfgs = [(n, ld)] * blocks
    E, blk = O.circuit_sizes(n, cfgs)
    return cfgs, rng.uniform(-np.pi, np.pi, size=(rows, E)), rng.uniform(-np.pi, np.pi, size=(blk, 3, n))


@pytest.mark.parametrize('n', [2, 3, 4, 5])
@pytest.mark.parametrize('readout', ['Z', 'X', 'Y', 'diag'])
def test_reference_equals_exact_values(n, readout):
    cfgs, x, w = _circuit(n, 3, ld=2 if n < 5 else 1, blocks=2, seed=n)
    kw = dict(offset=-0.4, coeff=1.3)
    if readout == 'diag':
        kw = dict(ham_diag=np.random.default_rng(n + 9).normal(size=1 << n))
    else:
        kw['ham_pauli'] = readout
    for p1, p2, q in ((0.03, 0.08, 0.04), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.2, 0.0, 0.5)):
        mean, var = NO.exact_values(n, cfgs, x, w, p1, p2, q, **kw)
        rmean, rvar = DR.exact_moments(n, cfgs, x, w, p1, p2, q, **kw)
        np.testing.assert_allclose(rmean, mean, rtol=0, atol=1e-13, err_msg=f'{p1} {p2} {q}')
        np.testing.assert_allclose(rvar, var, rtol=0, atol=1e-13, err_msg=f'{p1} {p2} {q}')


def test_reference_blocks_without_sublayers():
    """a block of encoding gates only (ld = 0): RX and its channel, nothing else"""
    n = 3
    cfgs = [(n, 0), (n, 1)]
    rng = np.random.default_rng(4)
    x, w = rng.uniform(-np.pi, np.pi, size=(2, 2 * n)), rng.uniform(-np.pi, np.pi, size=(1, 3, n))
    mean, var = NO.exact_values(n, cfgs, x, w, 0.05, 0.1, 0.02)
    rmean, rvar = DR.exact_moments(n, cfgs, x, w, 0.05, 0.1, 0.02)
    np.testing.assert_allclose(rmean, mean, rtol=0, atol=1e-13)
    np.testing.assert_allclose(rvar, var, rtol=0, atol=1e-13)
