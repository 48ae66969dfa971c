"""
CPU checks of the wide noisy forward (qhea_model_forward_noisy_wide, n = 7..12): the symbols, the library version and the
C ABI's host-side answers -- the workspace size and the argument checks.  Nothing is launched, no GPU needed.
"""
import ctypes
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 530 and _lib.MIN_LIB_VERSION >= 530
    for name in ('qhea_model_noisy_wide_workspace_bytes', 'qhea_model_forward_noisy_wide'):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert callable(_lib.model_forward_noisy_wide)


def _descs():
    from quanonet_amd import _lib
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (3, 1), 4, 0, True, 0.1, 0.0, 1.0)
    d12 = _lib.make_model_desc(_lib.MODEL_QUANONET, 12, (2, 1, 1, 2), 3, 2, True, 0.1, 0.0, 1.0)
    return d7, d12


def test_workspace_bytes(lib):
    from quanonet_amd import _lib
    size = lib.qhea_model_noisy_wide_workspace_bytes
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 150, 0)
    for d in _descs():
        for bad in (_lib.NoiseParams(-0.01, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.5, 0, 0, 1, 0),
                    _lib.NoiseParams(0, 0, 2.0, 0, 1, 0), _lib.NoiseParams(0, 0, 0, -3, 1, 0), _lib.NoiseParams(0, 0, 0, 0, 0, 0)):
            assert size(ctypes.byref(d), 100, ctypes.byref(bad)) == 0
        assert size(ctypes.byref(d), 100, None) == 0
        assert size(ctypes.byref(d), -1, ctypes.byref(ok)) == 0
        sizes = [size(ctypes.byref(d), b, ctypes.byref(ok)) for b in (0, 1, 37, 300, 5000)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[1]
        # 3 tiles of (sum, sum of squares) per row, and the two halves of the readout-confused table
        assert sizes[3] >= 300 * 3 * 16 + 2 * 8 * (1 << d.n_qubits)
    assert size(None, 100, ctypes.byref(ok)) == 0
    # n <= 6 belongs to qhea_model_forward_noisy
    d6 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 6, (3, 1), 4, 0, True, 0.1, 0.0, 1.0)
    assert size(ctypes.byref(d6), 100, ctypes.byref(ok)) == 0
    assert lib.qhea_model_noisy_workspace_bytes(ctypes.byref(d6), 100, ctypes.byref(ok)) > 0


def test_abi_argument_checks_without_gpu(lib):
    """the old call's list, in its order, with the qubit ranges exchanged"""
    from quanonet_amd import _lib
    call = lib.qhea_model_forward_noisy_wide
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0)
    d7, d12 = _descs()
    for d in (d7, d12):
        assert call(ctypes.byref(d), 0, 0, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == 0   # empty batch
        assert call(ctypes.byref(d), 0, 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1  # NULL inputs
        assert call(ctypes.byref(d), 0, -1, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1
        assert call(ctypes.byref(d), -1, 0, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1
        assert call(ctypes.byref(d), 0, 10, None, None, None, None, None, None, None, None, 0, None) == -1            # no noise setting
    d6 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 6, (3, 1), 4, 0, True, 0.1, 0.0, 1.0)
    assert call(ctypes.byref(d6), 0, 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -2
    # a bad noise setting is reported before the qubit count
    assert call(ctypes.byref(d6), 0, 10, None, None, None, None, ctypes.byref(_lib.NoiseParams(2.0, 0, 0, 0, 1, 0)), None, None,
                None, 0, None) == -1
    # X / Y read-outs do not combine with ham_diag (as in every other call)
    d7.ham_pauli = 1
    assert call(ctypes.byref(d7), 0, 10, None, None, None, ctypes.c_void_p(256), ctypes.byref(ok), None, None, None, 0,
                None) == -1
    # the old call keeps refusing what the wide one takes
    d7.ham_pauli = 0
    assert lib.qhea_model_forward_noisy(ctypes.byref(d7), 0, 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0,
                                        None) == -2
