"""
CPU checks of tests/device_traj_grad_reference.py, the numpy form of the quantum-jump trajectory gradient
(qhea_model_loss_grad_noisy_device): the adjoint walk against the exact two-term shift of the unnormalised numerator with the
pattern held fixed, the ideal limit, unbiasedness against the exact derivative of the density matrix (where the naive
derivative of the normalised value fails), the 2^-200 rescale, and the host side of the new entry points (nothing is launched).
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import hea_oracle as O
from tests import device_noise_grad_reference as DG
from tests import device_traj_grad_reference as G
from tests import device_traj_reference as TR
from tests.conftest import ROOT


def noise(n, rng, t1=1.0, strong=False):
    return dict(p1=list(rng.uniform(0.01, 0.06, n)), p2=list(rng.uniform(0.02, 0.08, n)), readout01=list(rng.uniform(0.0, 0.06, n)),
                readout10=list(rng.uniform(0.0, 0.08, n)), t1=list(rng.uniform(0.8, 1.5, n) * t1),
                t2=list(rng.uniform(0.6, 1.0, n) * t1), t_rx=0.1, t_rot=0.15, t_cx=0.25 if strong else 0.1, idle=True)


@pytest.mark.parametrize('n,cfgs,T', [(2, [(2, 2), (2, 1)], 6), (3, [(3, 1), (3, 2)], 5), (7, [(7, 1)], 3)])
def test_adjoint_walk_is_the_shift_of_the_numerator(n, cfgs, T):
    rng = np.random.default_rng(100 + n)
    B = 2
    x = rng.uniform(-2.0, 2.0, (B, n * len(cfgs)))
    w = rng.uniform(-np.pi, np.pi, (sum(ld for _, ld in cfgs), 3, n))
    nz = noise(n, rng, strong=True)
    diag = rng.normal(size=1 << n) if n == 3 else None
    pauli = {2: 'X', 3: 'Z', 7: 'Y'}[n]
    r = G.walk(n, cfgs, x, w, nz, T, 5, 0.3, 1.2, diag, pauli, row0=2)
    cov = G.coverage(r, n, T)
    assert cov['jumps'].sum() >= B * T and cov['pauli'] > 0 and cov['dephasing'] > 0, cov
    gx, gw = G.shift_grad(n, cfgs, x, w, nz, T, 5, 0.3, 1.2, diag, pauli, row0=2)
    err = max(np.abs(gx - r['gx']).max(), np.abs(gw - r['gw']).max())
    print(f'n={n}: jumps={int(cov["jumps"].sum())} max|adjoint - shift|={err:.2e}')
    assert err <= 1e-12
    # the value is the replay's
    v = TR.replay_values(n, cfgs, x, w, nz, 0, T, 5, 0.3, 1.2, diag, pauli, row0=2)
    np.testing.assert_allclose(r['value'].reshape(B, T), v, rtol=0, atol=1e-12)


def test_all_rates_zero_is_the_ideal_oracle():
    n, cfgs = 3, [(3, 2), (3, 1)]
    rng = np.random.default_rng(3)
    x = rng.uniform(-2.0, 2.0, (3, 6))
    w = rng.uniform(-np.pi, np.pi, (3, 3, n))
    z = [0.0] * n
    nz = dict(p1=z, p2=z, readout01=z, readout10=z, t1=[math.inf] * n, t2=[math.inf] * n, t_rx=0.1, t_rot=0.1, t_cx=0.1, idle=True)
    for pauli in ('Z', 'Y'):
        v, gx, gw = G.traj_grad(n, cfgs, x, w, nz, 2, 9, 0.5, 1.25, None, pauli)
        np.testing.assert_allclose(v, O.hea_forward(n, cfgs, x, w, 0.5, 1.25, None, pauli), rtol=0, atol=1e-12)
        _, ox, ow = O.hea_backward(n, cfgs, x, w, np.ones(3), 0.5, 1.25, None, pauli)
        np.testing.assert_allclose(gx, ox, rtol=0, atol=1e-12)
        np.testing.assert_allclose(gw.sum(axis=0), ow, rtol=0, atol=1e-12)


def test_unbiased_where_the_naive_derivative_is_not():
    """n = 2, one row, 3 sub-layers, gamma about 0.1 .. 0.3 per site (t / t1 = 0.1 .. 0.35), 40000 trajectories: every component
    of the mean of d num / N2 within 5 standard errors of the exact derivative of the density matrix
    (tests/device_noise_grad_reference.py); the derivative of the normalised value with the pattern fixed is tens of standard
    errors off.  Measured: worst z 1.99 (unbiased), 13.9 (naive)."""
    n, T = 2, 40000
    cfgs = [(n, 2), (n, 1)]
    rng = np.random.default_rng(11)
    x = rng.uniform(-2.0, 2.0, (1, 2 * n))
    w = rng.uniform(-np.pi, np.pi, (3, 3, n))
    nz = dict(p1=[0.02, 0.03], p2=[0.04, 0.03], readout01=[0.02, 0.05], readout10=[0.07, 0.03], t1=[1.0, 1.3], t2=[1.2, 0.9],
              t_rx=0.1, t_rot=0.15, t_cx=0.35, idle=True)
    assert TR.jump_pairs(n, nz)[..., 0].max() > 0.25
    ev, ex, ew = DG.circuit_grad(n, cfgs, x, w, nz, 0.5, 1.25)
    exact = np.concatenate([ex.reshape(-1), ew.reshape(-1)])
    worst = {}
    for naive in (False, True):
        r = G.walk(n, cfgs, x, w, nz, T, 21, 0.5, 1.25, naive=naive)
        g = np.concatenate([r['gx'], r['gw'].reshape(T, -1)], axis=1)
        mean, se = g.mean(axis=0), g.std(axis=0, ddof=1) / np.sqrt(T)
        z = np.abs(mean - exact) / np.maximum(se, 1e-300)
        z = np.where(np.abs(mean - exact) <= 1e-12, 0.0, z)
        worst[naive] = z.max()
        if not naive:
            zv = abs(r['value'].mean() - ev[0]) / (r['value'].std(ddof=1) / np.sqrt(T))
            assert zv <= 5.0 and r['counts']['jump'] > T
    print(f'worst z: d num / N2 {worst[False]:.2f}, naive {worst[True]:.2f}')
    assert worst[False] <= 5.0
    assert worst[True] > 5.0


def test_rescale_fires_and_is_crossed():
    """gamma = 1 - exp(-7) on 200 sub-layers of 3 wires: nearly every rotation site jumps and N2 falls by about a bit per jump,
    so the 2^-200 rescale fires; the adjoint walk crosses it and still is the shift of the numerator"""
    n, cfgs, T = 3, [(3, 200)], 2
    rng = np.random.default_rng(5)
    x = rng.uniform(-2.0, 2.0, (1, n))
    w = rng.uniform(-np.pi, np.pi, (200, 3, n))
    z = [0.0] * n
    nz = dict(p1=[0.01] * n, p2=z, readout01=z, readout10=z, t1=[1.0] * n, t2=[2.0] * n, t_rx=7.0, t_rot=7.0, t_cx=7.0, idle=False)
    r = G.walk(n, cfgs, x, w, nz, T, 1)
    jumps = G.coverage(r, n, T)['jumps']
    print(f'jumps per trajectory {jumps}, rescales {r["rescaled"]}, N2 {r["N2"]}')
    assert jumps.min() >= 200 and r['rescaled'].min() >= 1                # (about 300 jumps each)
    assert np.all(np.isfinite(r['gw'])) and np.abs(r['gw']).max() > 1e-3
    num = lambda ww: G.walk(n, cfgs, x, ww, nz, T, 1, forced=r['pattern'], grad=False)['num']
    for idx in [(0, 0, 0), (3, 1, 2), (50, 2, 1), (120, 1, 0), (199, 0, 0), (199, 2, 2)]:
        wp, wm = w.copy(), w.copy()
        wp[idx] += np.pi / 2
        wm[idx] -= np.pi / 2
        want = 0.5 * (num(wp) - num(wm)) / r['N2']
        got = r['gw'][(slice(None),) + idx]
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (idx, got, want)


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_host_side_of_the_entry_points(lib):
    """symbols, version, workspace sizes and every refusal that needs no device"""
    from quanonet_amd import _lib
    from tests.test_device_noise_abi import BAD, _record
    assert lib.qhea_version() >= 600 and _lib.MIN_LIB_VERSION >= 600
    for name in ('qhea_model_noisy_device_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_device',
                 'qhea_model_train_steps_noisy_device', 'qhea_device_noise_singular_site'):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    size, call = lib.qhea_model_noisy_device_grad_workspace_bytes, lib.qhea_model_loss_grad_noisy_device
    sp = _lib.SamplingParams(0, 5, 1)
    desc = lambda n: _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (2, 1), 4, 0, True, 0.1, 0.0, 1.0)
    for n in (7, 8, 9):
        assert size(ctypes.byref(desc(n)), 8, ctypes.byref(sp)) > 0
    for n in (6, 10):
        assert size(ctypes.byref(desc(n)), 8, ctypes.byref(sp)) == 0
    d = desc(7)
    for bad in (_lib.SamplingParams(1, 5, 1), _lib.SamplingParams(0, 0, 1), _lib.SamplingParams(-1, 5, 1)):
        assert size(ctypes.byref(d), 8, ctypes.byref(bad)) == 0
    assert size(ctypes.byref(d), 8, None) == 0 and size(ctypes.byref(d), -1, ctypes.byref(sp)) == 0
    # fixed size: a function of the shape, the batch and T only; the per-wave part stops growing at 2048 waves
    a, b, c, e = (size(ctypes.byref(d), B, ctypes.byref(_lib.SamplingParams(0, 64, 1))) for B in (64, 128, 256, 512))
    assert e - c == 2 * (c - b) > 0                                      # 2048 waves and more: rows only
    assert b - a > (c - b) // 2 + 1024 * 4096                            # 1024 more waves: a state per block each

    def run(dd, rec, samp, batch=4, row0=0):
        return call(ctypes.byref(dd), row0, batch, None, None, None, None, None, None if rec is None else ctypes.byref(rec),
                    None if samp is None else ctypes.byref(samp), 1.0, None, None, None, 0, None)
    ok = _record(7)
    assert run(d, ok, sp, batch=0) == 0
    assert run(d, ok, sp) == -1 and run(d, ok, sp, batch=-1) == -1 and run(d, ok, sp, row0=-1) == -1
    assert run(d, None, sp) == -1 and run(d, ok, None) == -1
    assert run(d, ok, _lib.SamplingParams(1, 5, 1), batch=0) == -1          # shot mode has no gradient
    assert run(d, ok, _lib.SamplingParams(0, 0, 1), batch=0) == -1
    for over in BAD:
        assert run(d, _record(7, **over), sp, batch=0) == -1, over
    for n in (6, 10):
        assert run(desc(n), _record(n), sp) == -2 and run(desc(n), _record(n), _lib.SamplingParams(1, 5, 1)) == -1
    # the site that cannot be walked back
    site, wire = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.qhea_device_noise_singular_site(7, ctypes.byref(ok), ctypes.byref(site), ctypes.byref(wire)) == 0
    from quanonet_amd.noise import DeviceNoise
    dead = DeviceNoise(t1=[1.0] * 6 + [1e-3], t2=[1.0] * 6 + [1e-3], t_rx=0.001, t_rot=0.001, t_cx=0.1, idle=False)
    rec = dead.params(7)
    assert lib.qhea_device_noise_singular_site(7, ctypes.byref(rec), ctypes.byref(site), ctypes.byref(wire)) == 1
    assert (site.value, wire.value) == (2, 6) and _lib.device_noise_singular_site(7, rec) == ('CTL', 6)
    assert lib.qhea_device_noise_singular_site(7, None, None, None) == -1


def test_python_surface_without_gpu():
    from quanonet_amd import noise as N
    from tests import helpers as H
    m6, m10 = H.heaqnn(6, 3, (1, 1), 0), H.heaqnn(10, 3, (1, 1), 0)
    dn, sp = N.DeviceNoise(p1=0.01), N.Sampling(trajectories=4)
    with pytest.raises(ValueError, match='device_noisy_loss_and_grad'):
        N.device_sampled_loss_and_grad(m6, None, None, dn, sp)
    with pytest.raises(ValueError, match='7..9'):
        N.device_sampled_loss_and_grad(m10, None, None, dn, sp)
    with pytest.raises(ValueError, match='shots'):
        N.device_sampled_loss_and_grad(H.heaqnn(7, 3, (1, 1), 0), None, None, dn, N.Sampling(shots=3))
    with pytest.raises(ValueError, match='DeviceNoise'):
        N.device_sampled_loss_and_grad(m6, None, None, N.NoiseModel(), sp)
    with pytest.raises(ValueError, match='Sampling'):
        N.device_sampled_loss_and_grad(m6, None, None, dn, N.NoiseModel())
