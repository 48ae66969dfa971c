"""
CPU checks of the device noise model (qhea_device_noise, quanonet_amd.noise.DeviceNoise): the host's folding of the model into
four channel sites per wire (qhea_device_noise_tables) against the triples read off the Kraus maps of
tests/device_noise_reference.py on a single qubit, the C ABI's argument checks (nothing is launched, no GPU needed), the
DeviceNoise class, and from_calibration on a hand-written calibration (tests/golden/device_calibration_5q.json, invented values
in the range a superconducting device reports).
"""
import ctypes
import dataclasses
import json
import math
import os
import subprocess

import numpy as np
import pytest

from tests import device_noise_reference as R
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 540 and _lib.MIN_LIB_VERSION >= 540
    for name in ('qhea_device_noise_tables', 'qhea_model_forward_noisy_device_exact'):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert callable(_lib.model_forward_noisy_device_exact) and callable(_lib.device_noise_tables)


def _random_noise(n, seed, idle=True, infinite=False):
    """per-wire parameters, all different; durations in units where T1 is of order one"""
    from quanonet_amd.noise import DeviceNoise
    rng = np.random.default_rng(seed)
    t1 = rng.uniform(0.8, 1.6, n)
    t2 = t1 * rng.uniform(0.5, 2.0, n)
    if infinite:
        t1, t2 = [math.inf] * n, [math.inf] * n
    return DeviceNoise(p1=rng.uniform(0.01, 0.05, n), p2=rng.uniform(0.02, 0.1, n), readout01=rng.uniform(0.01, 0.08, n),
                       readout10=rng.uniform(0.01, 0.08, n), t1=t1, t2=t2, t_rx=0.011, t_rot=0.017, t_cx=0.043, idle=idle)


def _site_triples(n, nz):
    """[4, n, 3] from the reference's Kraus maps, following one wire through a sub-layer slot by slot"""
    out = np.zeros((4, n, 3))
    for q in range(n):
        T1, T2, p1 = nz.t1[q], nz.t2[q], nz.p1[q]
        relax = lambda rho, t=nz.t_cx: R.relax_1q(rho, t, T1, T2)
        slots_before = [j for j in range(n) if q not in ((j + 1) % n, j) and j < (q - 1 if q >= 1 else 0)]
        # wire q >= 1 is control in slot q - 1 and target in slot q; wire 0 is target in slot 0 and control in slot n - 1
        after_target = [j for j in range(n) if q not in ((j + 1) % n, j) and j > q] if q >= 1 else \
            [j for j in range(1, n - 1)]
        if not nz.idle:
            slots_before, after_target = [], []

        def enc(rho):
            return R.relax_1q(R.apply_1q(rho, R.depolarizing_kraus(p1)), nz.t_rx, T1, T2)

        def rot(rho):
            rho = R.relax_1q(R.apply_1q(rho, R.depolarizing_kraus(p1)), nz.t_rot, T1, T2)
            for _ in slots_before:
                rho = relax(rho)
            return rho

        def tgt(rho):
            rho = relax(rho)
            for _ in after_target:
                rho = relax(rho)
            return rho
        for k, f in enumerate((enc, rot, relax, tgt)):
            out[k, q] = R.triple_of(f)
    return out


@pytest.mark.parametrize('n', [2, 3, 6])
@pytest.mark.parametrize('idle', [True, False])
def test_tables_match_the_kraus_maps(lib, n, idle):
    for infinite in (False, True):
        nz = _random_noise(n, seed=10 * n + idle, idle=idle, infinite=infinite)
        chan, lam2 = nz.tables(n)
        assert chan.shape == (4, n, 3) and lam2.shape == (n,)
        ref = _site_triples(n, nz)
        print(f'n={n} idle={idle} infinite={infinite}: max|chan err|={np.abs(chan - ref).max():.2e}')
        np.testing.assert_allclose(chan, ref, rtol=0, atol=1e-14)
        np.testing.assert_allclose(lam2, 16.0 * np.asarray(nz.p2) / 15.0, rtol=0, atol=1e-16)
        if infinite:                                                     # no decay: depolarizing at ENC / ROT, identity elsewhere
            k = 1.0 - 4.0 * np.asarray(nz.p1) / 3.0
            np.testing.assert_allclose(chan[:2], np.broadcast_to(np.stack([k, k, 0 * k], -1), (2, n, 3)), rtol=0, atol=1e-16)
            assert np.array_equal(chan[2:], np.broadcast_to([1.0, 1.0, 0.0], (2, n, 3)))


def test_idle_folding_by_hand(lib):
    """the site table of the header, entry by entry, at n = 4"""
    from quanonet_amd.noise import DeviceNoise
    n, T1, T2 = 4, 2.0, 3.0
    chan, _ = DeviceNoise(t1=T1, t2=T2, t_rx=0.1, t_rot=0.2, t_cx=0.3).tables(n)
    rel = lambda t: [math.exp(-t / T2), math.exp(-t / T1), 1.0 - math.exp(-t / T1)]
    for q in range(n):
        want = [rel(0.1), rel(0.2 + (max(q, 1) - 1) * 0.3), rel(0.3), rel((n - 1 if q == 0 else n - q) * 0.3)]
        np.testing.assert_allclose(chan[:, q], want, rtol=0, atol=1e-15, err_msg=f'wire {q}')


def _record(n, **over):
    from quanonet_amd.noise import DeviceNoise
    kw = dict(p1=[0.01] * n, p2=[0.02] * n, readout01=[0.03] * n, readout10=[0.04] * n, t1=[1.0] * n, t2=[1.5] * n,
              t_rx=0.01, t_rot=0.02, t_cx=0.03)
    rec = DeviceNoise(**kw).params(n)
    keep = []
    for k, v in over.items():
        if k in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2'):
            if v is None:
                setattr(rec, k, ctypes.POINTER(ctypes.c_double)())
            else:
                arr = (ctypes.c_double * n)(*v)
                keep.append(arr)
                setattr(rec, k, ctypes.cast(arr, ctypes.POINTER(ctypes.c_double)))
        else:
            setattr(rec, k, v)
    rec._keep = keep
    return rec


BAD = [dict(p1=None), dict(p2=None), dict(readout01=None), dict(readout10=None), dict(t1=None), dict(t2=None),
       dict(n_wires=4), dict(n_wires=0),
       dict(p1=[0.01, -0.1, 0.01, 0.01, 0.01]), dict(p2=[0.01, 0.01, 1.01, 0.01, 0.01]),
       dict(readout01=[0.01, 0.01, 0.01, 2.0, 0.01]), dict(readout10=[float('nan')] + [0.01] * 4),
       dict(p1=[float('nan')] * 5),
       dict(t_rx=-1e-9), dict(t_rot=float('nan')), dict(t_cx=-0.5), dict(t_cx=float('nan')),
       dict(t1=[1.0, 0.0, 1.0, 1.0, 1.0]), dict(t2=[1.0, 1.0, -2.0, 1.0, 1.0]), dict(t1=[float('nan')] + [1.0] * 4),
       dict(t2=[1.0, 1.0, 1.0, 1.0, float('nan')]),
       dict(t2=[1.5, 1.5, 1.5, 1.5, 2.0 + 1e-9]), dict(t1=[1.0] * 5, t2=[1.0, math.inf, 1.0, 1.0, 1.0])]


def test_abi_argument_checks_without_gpu(lib):
    from quanonet_amd import _lib
    call, tables = lib.qhea_model_forward_noisy_device_exact, lib.qhea_device_noise_tables
    n = 5
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    ok = _record(n)
    chan, lam2 = (ctypes.c_double * (4 * n * 3))(), (ctypes.c_double * n)()
    assert tables(n, ctypes.byref(ok), chan, lam2) == 0
    assert tables(n, ctypes.byref(ok), None, lam2) == -1 and tables(n, ctypes.byref(ok), chan, None) == -1
    assert tables(n, None, chan, lam2) == -1
    assert call(ctypes.byref(d), 0, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == 0   # empty batch
    assert call(ctypes.byref(d), -1, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1
    assert call(ctypes.byref(d), 10, None, None, None, None, None, None, None, None, 0, None) == -1     # no noise setting
    for over in BAD:
        bad = _record(n, **over)
        assert call(ctypes.byref(d), 10, None, None, None, None, ctypes.byref(bad), None, None, None, 0, None) == -1, over
        assert tables(n, ctypes.byref(bad), chan, lam2) == -1, over
    # T2 = 2 T1 exactly and infinite T1 with finite T2 are allowed
    for over in (dict(t1=[1.0] * 5, t2=[2.0] * 5), dict(t1=[math.inf] * 5, t2=[1.0] * 5), dict(t1=[math.inf] * 5, t2=[math.inf] * 5)):
        assert tables(n, ctypes.byref(_record(n, **over)), chan, lam2) == 0, over
    bad_desc = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    bad_desc.n_qubits = 0
    assert call(ctypes.byref(bad_desc), 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1
    # n >= 7: unsupported, and a bad setting is reported before the qubit count
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    assert call(ctypes.byref(d7), 10, None, None, None, None, ctypes.byref(_record(7)), None, None, None, 0, None) == -2
    assert call(ctypes.byref(d7), 10, None, None, None, None, ctypes.byref(_record(7, t_cx=-1.0)), None, None, None, 0,
                None) == -1
    assert call(ctypes.byref(d7), 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1   # 5 wires
    assert tables(7, ctypes.byref(_record(7)), (ctypes.c_double * 84)(), (ctypes.c_double * 7)()) == 0   # host only: any n
    # X / Y read-outs do not combine with ham_diag (as in every other call); NULL arrays of the call itself
    dx = _lib.make_model_desc(_lib.MODEL_QUANONET, 3, (1, 1, 1, 1), 4, 1, True, 0.1, 0.0, 1.0)
    dx.ham_pauli = 1
    assert call(ctypes.byref(dx), 10, None, None, None, ctypes.c_void_p(256), ctypes.byref(_record(3)), None, None, None, 0,
                None) == -1
    assert call(ctypes.byref(d), 10, None, None, None, None, ctypes.byref(ok), None, None, None, 0, None) == -1


def test_device_noise_validation():
    from quanonet_amd.noise import DeviceNoise
    DeviceNoise()
    DeviceNoise(p1=[0.1, 0.2], t1=[1.0, 2.0], t2=[2.0, 4.0], t_cx=1.0, idle=False)
    for kw in (dict(p1=-0.1), dict(p2=1.5), dict(readout01=[0.1, 2.0]), dict(readout10=float('nan')), dict(p1='a'), dict(p1=[]),
               dict(t1=0.0), dict(t2=-1.0), dict(t1=float('nan')), dict(t1=1.0, t2=2.5), dict(t1=[1.0, 1.0], t2=[1.0, 2.1]),
               dict(t2=1.0, t1=0.4), dict(t_rx=-1.0), dict(t_rot=float('nan')), dict(t_cx=math.inf), dict(idle=1),
               dict(p1=[0.1, 0.2], p2=[0.1, 0.2, 0.3]), dict(p1=True)):
        with pytest.raises(ValueError):
            DeviceNoise(**kw)
    with pytest.raises(ValueError):
        DeviceNoise(p1=[0.1, 0.2, 0.3]).params(4)                        # three entries, four wires
    rec = DeviceNoise(p1=[0.1, 0.2, 0.3], t1=5.0, t2=7.0, t_cx=0.25, idle=False).params(3)
    assert (rec.n_wires, rec.idle, rec.t_cx) == (3, 0, 0.25)
    assert [rec.p1[q] for q in range(3)] == [0.1, 0.2, 0.3] and [rec.t2[q] for q in range(3)] == [7.0] * 3
    with pytest.raises(dataclasses.FrozenInstanceError):
        DeviceNoise().p1 = 0.5


def test_uniform_and_asdict_round_trip(lib):
    from quanonet_amd.noise import DeviceNoise, NoiseModel
    u = DeviceNoise.uniform(NoiseModel(p1=0.03, p2=0.08, readout=0.04, shots=17, seed=3))
    assert (u.p1, u.p2, u.readout01, u.readout10, u.t1, u.t2, u.t_rx, u.t_rot, u.t_cx) == \
        (0.03, 0.08, 0.04, 0.04, math.inf, math.inf, 0.0, 0.0, 0.0)
    chan, lam2 = u.tables(4)
    k = 1.0 - 4.0 * 0.03 / 3.0
    assert np.array_equal(chan[:2], np.broadcast_to([k, k, 0.0], (2, 4, 3))) and np.array_equal(lam2, [16.0 * 0.08 / 15.0] * 4)
    for nz in (u, DeviceNoise(), _random_noise(5, 1), _random_noise(3, 2, idle=False, infinite=True),
               DeviceNoise(t1=[1.0, math.inf], t2=[2.0, 3.0], t_cx=0.5)):
        text = json.dumps(nz.asdict(), allow_nan=False)                  # strict JSON: no bare Infinity
        assert DeviceNoise.fromdict(json.loads(text)) == nz
    assert DeviceNoise().asdict()['t1'] == 'Infinity' and DeviceNoise(t1=[1.0, math.inf], t2=1.0).asdict()['t1'] == [1.0, 'Infinity']


def test_from_calibration(lib):
    from quanonet_amd.noise import DeviceNoise
    with open(os.path.join(GOLDEN, 'device_calibration_5q.json')) as f:
        cal = json.load(f)
    wires = [3, 4, 0, 1, 2]                                              # slot j: control wires[j + 1] -> target wires[j]
    nz = DeviceNoise.from_calibration(cal, wires)
    Q, P = cal['qubits'], cal['pairs']
    per = [Q[str(k)] for k in wires]
    edges = [P['3_4'], P['4_0'], P['0_1'], P['1_2'], P['2_3']]           # slot j joins wires[j] and wires[(j + 1) % 5]
    assert nz.p1 == tuple(1.0 - (1.0 - 1.5 * c['sx_error']) ** 2 for c in per)
    assert nz.p2 == tuple(1.25 * e['gate_error'] for e in edges)
    assert nz.readout01 == (0.027, 0.009, 0.012, 0.015, 0.020) and nz.readout10 == (0.027, 0.027, 0.030, 0.015, 0.048)
    assert nz.t1 == tuple(c['T1'] for c in per)
    assert nz.t2 == (2 * 6.4e-5, 1.05e-4, 9.5e-5, 1.31e-4, 6.2e-5)       # qubit 3 reports T2 > 2 T1: clipped
    assert nz.t_rx == nz.t_rot == 2 * 4.267e-8 and nz.t_cx == 5.3e-7 and nz.idle is True
    # the expected tables from the stated formulas
    chan, lam2 = nz.tables(5)
    for q in range(5):
        d = 1.0 - 4.0 * nz.p1[q] / 3.0
        rel = lambda t: np.array([math.exp(-t / nz.t2[q]), math.exp(-t / nz.t1[q]), 1.0 - math.exp(-t / nz.t1[q])])
        r_enc, r_rot = rel(nz.t_rx), rel(nz.t_rot + (max(q, 1) - 1) * nz.t_cx)
        np.testing.assert_allclose(chan[0, q], [r_enc[0] * d, r_enc[1] * d, r_enc[2]], rtol=0, atol=1e-15)
        np.testing.assert_allclose(chan[1, q], [r_rot[0] * d, r_rot[1] * d, r_rot[2]], rtol=0, atol=1e-15)
        np.testing.assert_allclose(chan[2, q], rel(nz.t_cx), rtol=0, atol=1e-15)
        np.testing.assert_allclose(chan[3, q], rel((4 if q == 0 else 5 - q) * nz.t_cx), rtol=0, atol=1e-15)
    np.testing.assert_allclose(lam2, [16.0 * p / 15.0 for p in nz.p2], rtol=0, atol=1e-17)
    three = DeviceNoise.from_calibration(cal, wires, pulses_rx=3, pulses_rot=3, idle=False)
    assert three.p1[0] == 1.0 - (1.0 - 1.5 * 4.4e-4) ** 3 and three.t_rx == 3 * 4.267e-8 and three.idle is False


def test_from_calibration_refuses_a_missing_edge(lib):
    from quanonet_amd.noise import DeviceNoise
    with open(os.path.join(GOLDEN, 'device_calibration_5q.json')) as f:
        cal = json.load(f)
    with pytest.raises(ValueError, match='ring edge'):
        DeviceNoise.from_calibration(cal, [0, 1, 3])                     # (1, 3) and (3, 0) are not coupled
    with pytest.raises(ValueError, match='ring edge'):
        DeviceNoise.from_calibration(cal, [0, 2])
    with pytest.raises(ValueError):
        DeviceNoise.from_calibration(cal, [0, 1, 7])                     # no such qubit
    assert DeviceNoise.from_calibration(cal, [1, 0]).p2 == (1.25 * 0.0071,) * 2      # a two-wire ring uses its one edge twice


def test_routing_refuses_what_cannot_honour_it():
    """the calls that sample Pauli errors or walk the uniform channels back say so, before they look at the model"""
    from quanonet_amd import noise as N
    from quanonet_amd.solver import _train_noise
    from tests import helpers as H
    dn = N.DeviceNoise(t1=1.0, t2=1.0, t_cx=0.1)
    m = H.heaqnn(2, 4, (3, 1), 0)
    for call in (lambda: N.noisy_predict(m, None, dn), lambda: N.amplification(m, dn),
                 lambda: N.exact_noisy_loss_and_grad(m, None, None, dn), lambda: _train_noise(dn)):
        with pytest.raises(ValueError, match='DeviceNoise'):
            call()
    assert N.amplification(m, N.NoiseModel(p1=0.01)) > 0.0               # a NoiseModel goes on as before
