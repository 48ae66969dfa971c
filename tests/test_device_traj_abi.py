"""
CPU checks of the quantum-jump trajectory call under the device noise model (qhea_model_forward_noisy_device,
quanonet_amd.noise.device_noisy_predict): the host's (gamma, pz) tables against the Kraus maps of
tests/device_noise_reference.py and against qhea_device_noise_tables, the Sampling record, the C ABI's argument checks
(nothing is launched, no GPU needed), the Python surface, and the numpy replay of tests/device_traj_reference.py -- the checker
the GPU tests compare the kernels with -- against the density-matrix reference.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import hea_oracle as O
from tests import device_noise_reference as R
from tests import device_traj_reference as TR
from tests.conftest import ROOT
from tests.test_device_noise_abi import BAD, _random_noise, _record


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def as_dict(dn, n):
    d = {k: [dn._at(k, q) for q in range(n)] for k in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2')}
    d.update(t_rx=dn.t_rx, t_rot=dn.t_rot, t_cx=dn.t_cx, idle=dn.idle)
    return d


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 560 and _lib.MIN_LIB_VERSION >= 560
    for name in ('qhea_device_noise_jump_tables', 'qhea_model_noisy_device_workspace_bytes', 'qhea_model_forward_noisy_device'):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert callable(_lib.model_forward_noisy_device) and callable(_lib.device_noise_jump_tables)
    assert ctypes.sizeof(_lib.SamplingParams) == 24


_PROBES = [np.array([[0.7, 0.2 - 0.1j], [0.2 + 0.1j, 0.3]]), np.array([[0, 1], [0, 0]], dtype=np.complex128),
           np.array([[0, 0], [0, 1]], dtype=np.complex128), np.eye(2, dtype=np.complex128)]


@pytest.mark.parametrize('n', [2, 5, 9, 12])
@pytest.mark.parametrize('idle', [True, False])
def test_jump_tables_match_the_kraus_maps(lib, n, idle):
    nz = _random_noise(n, seed=20 * n + idle, idle=idle)
    d = as_dict(nz, n)
    jump = nz.jump_tables(n)
    chan, _ = nz.tables(n)
    assert jump.shape == (4, n, 2)
    np.testing.assert_allclose(jump, TR.jump_pairs(n, d), rtol=0, atol=1e-15)
    worst = [0.0, 0.0]
    for site in range(4):
        for q in range(n):
            gamma, pz = jump[site, q]
            assert 0.0 <= gamma <= 1.0 and 0.0 <= pz <= 0.5
            tau = TR.site_duration(n, d, site, q)
            for rho in _PROBES:                                          # the three Kraus operators against AD-then-PD
                got, want = TR.site_channel(rho, gamma, pz), R.relax_1q(rho, tau, nz.t1[q], nz.t2[q])
                worst[0] = max(worst[0], np.abs(got - want).max())
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-14, err_msg=f'site {site} wire {q}')
            # D(p1[q]) then the site's relaxation is the (off, a, b) of qhea_device_noise_tables
            dep = (lambda r: R.apply_1q(r, R.depolarizing_kraus(nz.p1[q]))) if site < 2 else (lambda r: r)
            triple = R.triple_of(lambda r: TR.site_channel(dep(r), gamma, pz))
            worst[1] = max(worst[1], np.abs(triple - chan[site, q]).max())
            np.testing.assert_allclose(triple, chan[site, q], rtol=0, atol=1e-14, err_msg=f'site {site} wire {q}')
    print(f'n={n} idle={idle}: max|channel err|={worst[0]:.2e} max|triple err|={worst[1]:.2e}')


def test_jump_table_edges(lib):
    from quanonet_amd.noise import DeviceNoise
    n = 3
    # no relaxation at all: every site is the identity
    assert np.array_equal(DeviceNoise(t_rx=0.1, t_rot=0.2, t_cx=0.3).jump_tables(n), np.zeros((4, n, 2)))
    # zero durations with finite times
    assert np.array_equal(DeviceNoise(t1=1.0, t2=1.0).jump_tables(n), np.zeros((4, n, 2)))
    # infinite t1, finite t2: pure dephasing, pz = (1 - exp(-t / t2)) / 2
    j = DeviceNoise(t1=math.inf, t2=2.0, t_rx=0.1, t_rot=0.1, t_cx=0.1, idle=False).jump_tables(n)
    assert np.all(j[..., 0] == 0.0)
    np.testing.assert_allclose(j[..., 1], 0.5 * (1.0 - math.exp(-0.05)), rtol=0, atol=1e-16)
    # t2 = 2 t1: no pure dephasing beyond what damping does (pz = 0 to rounding, never negative)
    j = DeviceNoise(t1=1.5, t2=3.0, t_rx=0.1, t_rot=0.2, t_cx=0.3).jump_tables(n)
    assert np.all(j[..., 0] > 0.0) and np.all(j[..., 1] >= 0.0) and np.all(j[..., 1] < 1e-15)
    # tau / t1 > 745: exp underflows, gamma = 1, pz = 1/2, nothing is NaN
    j = DeviceNoise(t1=1.0, t2=1.0, t_rx=800.0, t_rot=800.0, t_cx=800.0).jump_tables(n)
    assert np.all(np.isfinite(j)) and np.all(j[..., 0] == 1.0) and np.all(j[..., 1] == 0.5)


def test_sampling_record():
    from quanonet_amd.noise import Sampling
    s = Sampling()
    assert (s.shots, s.trajectories, s.seed) == (0, 1, 0)
    assert Sampling(shots=5, trajectories=0).asdict() == {'shots': 5, 'trajectories': 0, 'seed': 0}
    p = Sampling(shots=3, trajectories=7, seed=(1 << 64) - 1).params()
    assert (p.shots, p.trajectories, p.seed) == (3, 7, (1 << 64) - 1)
    for bad in (dict(shots=-1), dict(trajectories=0), dict(seed=-1), dict(seed=1 << 64), dict(shots=1.0), dict(trajectories=True),
                dict(seed='0')):
        with pytest.raises(ValueError, match='Sampling'):
            Sampling(**bad)
    with pytest.raises(Exception):
        s.shots = 3                                                      # frozen


def test_abi_argument_checks_without_gpu(lib):
    from quanonet_amd import _lib
    call, tables, ws_bytes = (lib.qhea_model_forward_noisy_device, lib.qhea_device_noise_jump_tables,
                              lib.qhea_model_noisy_device_workspace_bytes)
    n = 5
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    ok, sp = _record(n), _lib.SamplingParams(0, 3, 1)
    jump = (ctypes.c_double * (4 * n * 2))()
    assert tables(n, ctypes.byref(ok), jump) == 0
    assert tables(n, ctypes.byref(ok), None) == -1 and tables(n, None, jump) == -1
    for over in BAD:
        assert tables(n, ctypes.byref(_record(n, **over)), jump) == -1, over
    for m in (1, 13):
        assert tables(m, ctypes.byref(_record(m)), (ctypes.c_double * (8 * m))()) == -1
    assert tables(12, ctypes.byref(_record(12)), (ctypes.c_double * 96)()) == 0      # host arithmetic: wider than the kernels

    def run(desc, rec, samp, batch=4, row0=0):
        return call(ctypes.byref(desc), row0, batch, None, None, None, None, None if rec is None else ctypes.byref(rec),
                    None if samp is None else ctypes.byref(samp), None, None, None, 0, None)
    assert run(d, ok, sp, batch=0) == 0                                  # empty batch
    assert run(d, ok, sp, batch=-1) == -1 and run(d, ok, sp, row0=-1) == -1
    assert run(d, ok, sp) == -1                                          # NULL arrays
    assert run(d, None, sp) == -1 and run(d, ok, None) == -1
    for over in BAD:
        assert run(d, _record(n, **over), sp, batch=0) == -1, over
    bad_sampling = [_lib.SamplingParams(-1, 1, 0), _lib.SamplingParams(0, 0, 0), _lib.SamplingParams(0, -5, 0),
                    _lib.SamplingParams(1 << 32, 1, 0), _lib.SamplingParams(0, 1 << 32, 0)]
    for bad in bad_sampling:
        assert run(d, ok, bad, batch=0) == -1
        assert ws_bytes(ctypes.byref(d), 8, ctypes.byref(bad)) == 0
    assert run(d, ok, _lib.SamplingParams((1 << 32) - 1, 0, 0), batch=0) == 0
    assert ws_bytes(ctypes.byref(d), 8, ctypes.byref(sp)) > 0
    assert ws_bytes(ctypes.byref(d), 8, None) == 0 and ws_bytes(ctypes.byref(d), -1, ctypes.byref(sp)) == 0
    bad_desc = _lib.make_model_desc(_lib.MODEL_QUANONET, 1, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    assert ws_bytes(ctypes.byref(bad_desc), 8, ctypes.byref(sp)) == 0
    # more tiles, more workspace; shot mode has no trajectories to count
    assert ws_bytes(ctypes.byref(d), 8, ctypes.byref(_lib.SamplingParams(0, 1000, 0))) > ws_bytes(ctypes.byref(d), 8, ctypes.byref(sp))
    # n = 10..12: the setting and the sampling record are checked first, then the call is unsupported
    d10 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 10, (2, 1), 4, 0, True, 0.1, 0.0, 1.0)
    assert run(d10, _record(10), sp) == -2 and run(d10, _record(10), sp, batch=0) == -2
    assert run(d10, _record(10, t_cx=-1.0), sp) == -1 and run(d10, _record(10), bad_sampling[1]) == -1
    assert ws_bytes(ctypes.byref(d10), 8, ctypes.byref(sp)) == 0
    d9 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 9, (2, 1), 4, 0, True, 0.1, 0.0, 1.0)
    assert run(d9, _record(9), sp, batch=0) == 0 and ws_bytes(ctypes.byref(d9), 8, ctypes.byref(sp)) > 0
    assert run(d, _record(4), sp, batch=0) == -1                         # n_wires != n


def test_python_surface_without_gpu():
    from quanonet_amd import noise as N
    from tests import helpers as H
    m = H.quanonet(3, 3, 2, (2, 1, 1, 2), 0)
    with pytest.raises(ValueError, match='noisy_predict'):
        N.device_noisy_predict(m, None, N.NoiseModel(), N.Sampling())
    with pytest.raises(ValueError, match='Sampling'):
        N.device_noisy_predict(m, None, N.DeviceNoise(), N.NoiseModel())
    with pytest.raises(ValueError, match='DeviceNoise') as e:
        N.noisy_predict(m, None, N.DeviceNoise())
    assert 'device_noisy_predict' in str(e.value) and 'sampling=' in str(e.value)
    with pytest.raises(ValueError, match='DeviceNoise'):
        N.amplification(m, N.DeviceNoise())
    with pytest.raises(ValueError, match='9 entries'):
        N.DeviceNoise(p1=[0.1] * 9).jump_tables(8)


@pytest.mark.parametrize('shots', [0, 1])
def test_replay_is_unbiased_for_the_density_matrix(shots):
    """n = 2, one row, depth (2 blocks of 1 sub-layer), strong relaxation: 20000 replayed trajectories against the exact value
    of tests/device_noise_reference.py.  z = (mean - exact) / stderr; |z| <= 5."""
    n, T = 2, 20000
    rng = np.random.default_rng(7)
    cfgs = [(n, 1), (n, 1)]
    x = rng.uniform(-2.0, 2.0, (1, 2 * n))
    w = rng.uniform(-np.pi, np.pi, (2, 3, n))
    nz = dict(p1=[0.03, 0.05], p2=[0.08, 0.06], readout01=[0.02, 0.05], readout10=[0.07, 0.03], t1=[1.0, 1.4], t2=[1.2, 0.9],
              t_rx=0.1, t_rot=0.15, t_cx=0.3, idle=True)
    for ham_pauli, diag in (('Z', None), ('X', None), ('Z', rng.normal(size=1 << n))):
        counts = {}
        vals = TR.replay_values(n, cfgs, x, w, nz, shots * T, T, 11, offset=0.5, coeff=1.25, ham_diag=diag, ham_pauli=ham_pauli,
                                row0=3, counts=counts)
        assert vals.shape == (1, T) and counts['jump'] > T // 4 and counts['dephasing'] > T // 20 and counts['pauli'] > T // 10
        mean, se = TR.mean_and_stderr(vals)
        exact, var = R.device_moments(n, cfgs, x, w, nz, 0.5, 1.25, diag, ham_pauli)
        z = (mean[0] - exact[0]) / se[0]
        print(f'shots={shots} {ham_pauli} diag={diag is not None}: mean={mean[0]:.5f} exact={exact[0]:.5f} z={z:.2f} '
              f'std ratio={se[0] * np.sqrt(T) / np.sqrt(var[0]) if shots else float("nan"):.3f}')
        assert abs(z) <= 5.0
        if shots:                                                        # one shot's deviation is the exact one (1 % at T = 20000)
            assert abs(se[0] * np.sqrt(T) / np.sqrt(var[0]) - 1.0) < 0.05
        # the ideal setting replays the ideal circuit
    ideal = dict(nz, p1=[0, 0], p2=[0, 0], readout01=[0, 0], readout10=[0, 0], t1=[math.inf] * 2, t2=[math.inf] * 2)
    v = TR.replay_values(n, cfgs, x, w, ideal, 0, 3, 11, offset=0.5, coeff=1.25)
    np.testing.assert_allclose(v, np.broadcast_to(O.hea_forward(n, cfgs, x, w, 0.5, 1.25)[:, None], (1, 3)), rtol=0, atol=1e-13)
