"""
CPU checks of the noisy-forward checker (tests/noise_oracle.py), the NoiseModel settings and the C ABI's argument checks of
qhea_model_forward_noisy (no kernel is launched, no GPU needed).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import hea_oracle as O
from tests import noise_oracle as NO
from tests.conftest import ROOT

# Random123's kat_vectors for philox4x32_10
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


class Noise:
    def __init__(self, p1=0.0, p2=0.0, readout=0.0, shots=0, trajectories=1, seed=0):
        self.p1, self.p2, self.readout, self.shots, self.trajectories, self.seed = p1, p2, readout, shots, trajectories, seed


def _circuit(n, rows, ld=1, blocks=2, seed=0):
    rng = np.random.default_rng(seed)
    cfgs = [(n, ld)] * blocks
    E, blk = O.circuit_sizes(n, cfgs)
    return cfgs, rng.uniform(-np.pi, np.pi, size=(rows, E)), rng.uniform(-np.pi, np.pi, size=(blk, 3, n))


@pytest.mark.parametrize('ctr,key,out', KAT)
def test_philox_known_answers(ctr, key, out):
    words = NO.philox4x32(ctr, key)
    assert tuple(int(w[0]) for w in words) == out


def test_philox_vectorised_matches_scalar():
    c = np.arange(5, dtype=np.uint64)
    many = NO.philox4x32((c, 7, 11, 0), (3, 4))
    for i in range(5):
        one = NO.philox4x32((i, 7, 11, 0), (3, 4))
        assert tuple(int(w[i]) for w in many) == tuple(int(w[0]) for w in one)


def test_noiseless_replay_is_the_ideal_forward():
    n = 3
    cfgs, x, w = _circuit(n, 5)
    for pauli in ('Z', 'X', 'Y'):
        v = NO.replay_values(n, cfgs, x, w, Noise(), offset=0.3, coeff=0.7, ham_pauli=pauli)
        ref = O.hea_forward(n, cfgs, x, w, 0.3, 0.7, ham_pauli=pauli)
        np.testing.assert_allclose(v[:, 0], ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize('shots', [0, 3000])
def test_replay_mean_matches_density_matrix_n2(shots):
    n = 2
    cfgs, x, w = _circuit(n, 3, ld=2)
    nz = Noise(p1=0.05, p2=0.1, readout=0.04, shots=shots, trajectories=3000, seed=12345)
    v = NO.replay_values(n, cfgs, x, w, nz, offset=-0.2, coeff=1.3)
    mean, _ = NO.exact_values(n, cfgs, x, w, nz.p1, nz.p2, nz.readout, offset=-0.2, coeff=1.3)
    se = v.std(axis=1, ddof=1) / np.sqrt(v.shape[1])
    assert np.all(se > 0)
    assert np.all(np.abs(v.mean(axis=1) - mean) < 5 * se), (v.mean(axis=1), mean, se)


def test_replay_y_readout_matches_density_matrix():
    n = 2
    cfgs, x, w = _circuit(n, 2, ld=1, seed=3)
    nz = Noise(p1=0.1, p2=0.2, readout=0.05, trajectories=3000, seed=99)
    v = NO.replay_values(n, cfgs, x, w, nz, offset=0.0, coeff=1.0, ham_pauli='Y')
    mean, _ = NO.exact_values(n, cfgs, x, w, nz.p1, nz.p2, nz.readout, ham_pauli='Y')
    se = v.std(axis=1, ddof=1) / np.sqrt(v.shape[1])
    assert np.all(np.abs(v.mean(axis=1) - mean) < 5 * se)


def test_readout_diag_against_density_matrix_readout():
    n = 3
    cfgs, x, w = _circuit(n, 4, seed=5)
    diag = np.random.default_rng(1).normal(size=1 << n)
    for q in (0.0, 0.03, 0.5, 1.0):
        v = NO.replay_values(n, cfgs, x, w, Noise(readout=q), ham_diag=diag)
        mean, _ = NO.exact_values(n, cfgs, x, w, 0.0, 0.0, q, ham_diag=diag)
        np.testing.assert_allclose(v[:, 0], mean, rtol=0, atol=1e-12)
    # q = 0 is the identity, q = 1 reads every bit flipped
    np.testing.assert_array_equal(NO.readout_diag(diag, n, 0.0), diag)
    np.testing.assert_allclose(NO.readout_diag(diag, n, 1.0), diag[::-1], rtol=0, atol=0)


def test_noise_model_validation():
    from quanonet_amd.noise import NoiseModel
    nm = NoiseModel(p1=0.01, p2=0.02, readout=0.03, shots=100, trajectories=1, seed=(1 << 64) - 1)
    p = nm.params()
    assert (p.p1, p.p2, p.readout, p.shots, p.trajectories, p.seed) == (0.01, 0.02, 0.03, 100, 1, (1 << 64) - 1)
    assert nm.asdict()['shots'] == 100
    assert NoiseModel() == NoiseModel(0.0, 0.0, 0.0, 0, 1, 0)
    with pytest.raises(Exception):
        nm.p1 = 0.5                                          # frozen
    for bad in (dict(p1=-0.1), dict(p2=1.5), dict(readout=float('nan')), dict(shots=-1), dict(trajectories=0),
                dict(seed=-1), dict(seed=1 << 64), dict(shots=1.5)):
        with pytest.raises(ValueError):
            NoiseModel(**bad)
    NoiseModel(shots=10, trajectories=0)                     # trajectories are ignored in shot mode
    NoiseModel(p1=1.0, p2=1.0, readout=1.0)


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_abi_argument_checks_without_gpu(lib):
    from quanonet_amd import _lib
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, 5, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    ok = _lib.NoiseParams(0.01, 0.02, 0.0, 0, 4, 7)
    assert lib.qhea_model_noisy_workspace_bytes(ctypes.byref(d), 100, ctypes.byref(ok)) > 100 * 10 * 16
    assert lib.qhea_model_forward_noisy(ctypes.byref(d), 0, 0, None, None, None, None, ctypes.byref(ok), None, None, None, 0,
                                        None) == 0                 # empty batch
    for bad in (_lib.NoiseParams(-0.1, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.01, 0, 0, 1, 0),
                _lib.NoiseParams(0, 0, float('nan'), 0, 1, 0), _lib.NoiseParams(0, 0, 0, -1, 1, 0),
                _lib.NoiseParams(0, 0, 0, 0, 0, 0)):
        assert lib.qhea_model_noisy_workspace_bytes(ctypes.byref(d), 10, ctypes.byref(bad)) == 0
        assert lib.qhea_model_forward_noisy(ctypes.byref(d), 0, 10, None, None, None, None, ctypes.byref(bad), None, None,
                                            None, 0, None) == -1
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    assert lib.qhea_model_forward_noisy(ctypes.byref(d7), 0, 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0,
                                        None) == -2
    assert lib.qhea_model_forward_noisy(ctypes.byref(d), -1, 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0,
                                        None) == -1                # negative row0
