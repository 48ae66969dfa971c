"""
CPU checks of training under the calibrated device noise model (qhea_model_loss_grad_noisy_device_exact /
qhea_model_train_steps_noisy_device_exact): the symbols, the guard's log10 A_dev against the uniform call and against the numpy
helper, the C ABI's argument checks (nothing is launched, no GPU needed), the helper tests/device_noise_grad_reference.py against
itself (stored walk, inverse walk, parameter shift) and against torch autograd for the model's chain rule, the conditioning
probe that fixes the guard's bound, and the parsing of the config key train_device_noise.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from tests import density_grad_reference as DG
from tests import device_noise_grad_reference as DV
from tests import helpers as H
from tests.conftest import ROOT
from tests.test_device_noise_abi import BAD, _record
from tests.test_noisy_forward import _model

NEW = ('qhea_model_device_noisy_grad_workspace_bytes', 'qhea_model_device_noisy_log10_amplification',
       'qhea_model_loss_grad_noisy_device_exact', 'qhea_model_train_steps_noisy_device_exact')
MAX_LOG10_AMPLIFICATION = 7.0           # kMaxLog10AmplificationDevice of the library, the bound the probe below justifies


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def device_noise(n, idle, seed=0, scale=1.0, infinite_wire=1):
    """every wire's p1, p2, readout01 / readout10, T1 and T2 different, wire `infinite_wire` without relaxation; `scale`
    multiplies the rates and the durations (1: p1 in [0.01, 0.05], p2 in [0.02, 0.1], t / T1 per layer in [0.01, 0.05])"""
    from quanonet_amd.noise import DeviceNoise
    rng = np.random.default_rng(2000 + 10 * n + seed)
    t1 = rng.uniform(1.0, 2.0, n)
    t2 = t1 * rng.uniform(0.5, 2.0, n)
    if infinite_wire is not None:
        t1[infinite_wire % n] = t2[infinite_wire % n] = math.inf
    return DeviceNoise(p1=scale * rng.uniform(0.01, 0.05, n), p2=scale * rng.uniform(0.02, 0.1, n),
                       readout01=rng.uniform(0.01, 0.08, n), readout10=rng.uniform(0.01, 0.08, n), t1=t1, t2=t2,
                       t_rx=0.02 * scale, t_rot=0.03 * scale, t_cx=0.05 * scale, idle=idle)


def as_dict(dn, n):
    """a DeviceNoise as the dict the numpy references take"""
    d = {k: [dn._at(k, q) for q in range(n)] for k in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2')}
    d.update(t_rx=dn.t_rx, t_rot=dn.t_rot, t_cx=dn.t_cx, idle=dn.idle)
    return d


def _cfgs(d):
    net = tuple(d.net)
    return O.block_configs_quanonet(d.n_qubits, net) if d.model == 0 else O.block_configs_heaqnn(d.n_qubits, net[:2])


def _amp(lib, d, rec):
    return lib.qhea_model_device_noisy_log10_amplification(ctypes.byref(d), ctypes.byref(rec))


def _shapes(n):
    from quanonet_amd import _lib
    return [_lib.make_model_desc(_lib.MODEL_QUANONET, n, (3, 2, 2, 1), 4, 1, True, 0.1, 0.0, 1.0),
            _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (4, 3), 4, 0, False, 0.1, 0.0, 1.0),
            _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 0, 1, 2), 4, 1, True, 0.1, 0.0, 1.0)]


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 550 and _lib.MIN_LIB_VERSION >= 550
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    for f in (_lib.model_loss_grad_noisy_device_exact, _lib.model_train_steps_noisy_device_exact,
              _lib.model_device_noisy_log10_amplification):
        assert callable(f)
    from quanonet_amd.noise import device_amplification, device_noisy_loss_and_grad
    assert callable(device_amplification) and callable(device_noisy_loss_and_grad)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
def test_guard_reduces_to_the_uniform_one(lib, n):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise, NoiseModel
    for d in _shapes(n):
        for p1, p2, ro in ((0.0, 0.0, 0.0), (1e-3, 1e-2, 1e-2), (0.03, 0.08, 0.04), (0.2, 0.5, 0.3), (0.0, 0.3, 0.0), (0.4, 0.0, 1.0)):
            nm = NoiseModel(p1=p1, p2=p2, readout=ro)
            want = lib.qhea_model_exact_noisy_log10_amplification(ctypes.byref(d), ctypes.byref(nm.params()))
            got = _amp(lib, d, DeviceNoise.uniform(nm).params(n))
            assert abs(got - want) <= 1e-12, (n, tuple(d.net), p1, p2, got, want)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('idle', [True, False])
def test_guard_against_the_helper(lib, n, idle):
    for seed, d in enumerate(_shapes(n)):
        dn = device_noise(n, idle, seed=seed)
        got = _amp(lib, d, dn.params(n))
        nz, cfgs = as_dict(dn, n), _cfgs(d)
        from_tables = DV.log10_amplification(n, cfgs, nz, tables=dn.tables(n))
        from_kraus = DV.log10_amplification(n, cfgs, nz)
        print(f'n={n} idle={idle} net={tuple(d.net)}: log10 A_dev={got:.6f} (helper {from_tables:.6f})')
        assert abs(got - from_tables) <= 1e-12 and abs(got - from_kraus) <= 1e-12 and got > 0.0


def test_guard_special_values(lib):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    n = 4
    d = _shapes(n)[0]
    ok = dict(p1=[0.01] * n, p2=[0.02] * n, t1=[1.0] * n, t2=[1.5] * n, t_rx=0.01, t_rot=0.02, t_cx=0.03)
    base = _amp(lib, d, DeviceNoise(**ok).params(n))
    assert 0.0 < base < MAX_LOG10_AMPLIFICATION
    # singular channels: +inf, and the calls refuse them before they look at the (empty) batch
    for over in (dict(p1=[0.01, 0.75, 0.01, 0.01]), dict(p2=[0.02, 0.02, 15 / 16, 0.02]), dict(t_cx=1e4), dict(p1=[1.0] * n)):
        rec = DeviceNoise(**dict(ok, **over)).params(n)
        assert _amp(lib, d, rec) == math.inf, over
        assert _loss_grad(lib, d, 0, rec) == -2 and _train_steps(lib, d, 0, rec) == -2, over
    # NaN: a bad descriptor, a setting for another number of wires, a refused setting, no setting
    bad_desc = _shapes(n)[0]
    bad_desc.n_qubits = 0
    assert math.isnan(_amp(lib, bad_desc, DeviceNoise(**ok).params(n)))
    assert math.isnan(_amp(lib, d, DeviceNoise().params(n + 1)))
    assert math.isnan(_amp(lib, d, _record(n, t_cx=-1.0)))
    assert math.isnan(lib.qhea_model_device_noisy_log10_amplification(ctypes.byref(d), None))
    assert math.isnan(lib.qhea_model_device_noisy_log10_amplification(None, ctypes.byref(DeviceNoise().params(n))))
    # relaxation adds to it: strictly larger with finite T1 than without, and with the idle decay than without it
    no_t1 = _amp(lib, d, DeviceNoise(**dict(ok, t1=[math.inf] * n)).params(n))
    assert base > no_t1 > _amp(lib, d, DeviceNoise(**dict(ok, t1=[math.inf] * n, t2=[math.inf] * n)).params(n)) > 0.0
    assert base > _amp(lib, d, DeviceNoise(idle=False, **ok).params(n))
    assert _amp(lib, d, DeviceNoise().params(n)) == 0.0
    # a long t_cx trips the bound without any singular channel: refused above it, accepted below
    lo, hi = 0.0, 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _amp(lib, d, DeviceNoise(**dict(ok, t_cx=mid)).params(n)) < MAX_LOG10_AMPLIFICATION else (lo, mid)
    above, below = DeviceNoise(**dict(ok, t_cx=hi * 1.001)).params(n), DeviceNoise(**dict(ok, t_cx=lo * 0.999)).params(n)
    assert MAX_LOG10_AMPLIFICATION < _amp(lib, d, above) < MAX_LOG10_AMPLIFICATION + 0.05
    assert MAX_LOG10_AMPLIFICATION - 0.05 < _amp(lib, d, below) < MAX_LOG10_AMPLIFICATION
    assert _loss_grad(lib, d, 0, above) == -2 and _train_steps(lib, d, 0, above) == -2 and _loss_grad(lib, d, 10, above) == -2
    assert _loss_grad(lib, d, 0, below) == 0 and _train_steps(lib, d, 0, below) == 0
    assert _loss_grad(lib, d, 10, below) == -1                                    # reaches the NULL arrays


def _loss_grad(lib, d, batch, rec, ham_diag=None):
    """the call with every array NULL: what the checks in front of the pointers return"""
    return lib.qhea_model_loss_grad_noisy_device_exact(None if d is None else ctypes.byref(d), batch, None, None, None, None,
                                                       ham_diag, None if rec is None else ctypes.byref(rec), 1.0, None, None,
                                                       None, 0, None)


def _train_steps(lib, d, n_steps, rec, first_step=1):
    return lib.qhea_model_train_steps_noisy_device_exact(None if d is None else ctypes.byref(d), n_steps, None, None, None, None,
                                                         None, None, None if rec is None else ctypes.byref(rec), None, None, 0,
                                                         None, None, first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, 0, None)


def test_abi_argument_checks_without_gpu(lib):
    from quanonet_amd import _lib
    n = 5
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    ok = _record(n)
    # the uniform gradient call's workspace and the table of the channel forms (66 doubles per wire, six wires)
    uni = lib.qhea_model_exact_noisy_grad_workspace_bytes(ctypes.byref(d), 100)
    assert lib.qhea_model_device_noisy_grad_workspace_bytes(ctypes.byref(d), 100) >= uni + 6 * 66 * 8
    assert lib.qhea_model_device_noisy_grad_workspace_bytes(ctypes.byref(d), -1) == 0
    assert lib.qhea_model_device_noisy_grad_workspace_bytes(None, 100) == 0
    bad_desc = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    bad_desc.n_qubits = 0
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    for call in (_loss_grad, _train_steps):
        assert call(lib, bad_desc, 10, ok) == -1
        assert call(lib, None, 10, ok) == -1
        assert call(lib, d, 0, ok) == 0                                           # empty batch / no steps
        assert call(lib, d, 10, None) == -1                                       # no setting
        for over in BAD:                                                          # every EINVAL setting of the forward call
            assert call(lib, d, 10, _record(n, **over)) == -1, over
            assert call(lib, d, 0, _record(n, **over)) == -1, over                # ... before the empty batch is looked at
        assert call(lib, d, -1, ok) == -1
        assert call(lib, d7, 10, _record(7)) == -2
        assert call(lib, d7, 10, _record(7, t_cx=-1.0)) == -1                     # a bad setting is reported before the qubit count
        assert call(lib, d7, 10, ok) == -1                                        # 5 wires for 7 qubits
        assert call(lib, d, 10, ok) == -1                                         # valid up to the NULL arrays
    assert _train_steps(lib, d, 3, ok, first_step=0) == -1
    # X / Y read-outs do not combine with ham_diag (as in every other call)
    dx = _lib.make_model_desc(_lib.MODEL_QUANONET, 3, (1, 1, 1, 1), 4, 1, True, 0.1, 0.0, 1.0)
    dx.ham_pauli = 1
    assert _loss_grad(lib, dx, 10, _record(3), ham_diag=ctypes.cast(ctypes.c_void_p(256), ctypes.POINTER(ctypes.c_double))) == -1


def test_train_steps_two_faults_at_once(lib):
    """which code wins: unlike the uniform call, first_step = 0 is reported after the setting, the qubit count, the guard and
    the shared checks, and before the return of a call without steps (the codes are those of the library before its entry
    points shared one body)"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    from tests.test_noise_aware_abi import full_train_steps
    n = 5
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    ok, bad = _record(n), _record(n, t_cx=-1.0)
    singular = DeviceNoise(p1=[0.01] * n, p2=[0.02] * n, t1=[1.0] * n, t2=[1.5] * n, t_rx=0.01, t_rot=0.02, t_cx=1e4).params(n)
    name = 'qhea_model_train_steps_noisy_device_exact'
    table = [('first_step 0, no row_begin', dict(d=d, nz=ok, first_step=0, row_begin=False), -1),
             ('first_step 0, invalid setting', dict(d=d, nz=bad, first_step=0), -1),
             ('first_step 0, n = 7', dict(d=d7, nz=_record(7), first_step=0), -2),
             ('first_step 0, refused amplification', dict(d=d, nz=singular, first_step=0), -2),
             ('first_step 0, no steps', dict(d=d, nz=ok, first_step=0, n_steps=0), -1),
             ('no steps alone', dict(d=d, nz=ok, n_steps=0), 0),
             ('no workspace, a valid call of two steps', dict(d=d, nz=ok), -3)]
    for what, kw, want in table:
        assert full_train_steps(lib, name, **kw) == want, what


def _circuit_case(n, kind, readout, seed):
    """(cfgs, x, w, read-out kwargs) of a small circuit with blocks of depth 0, 1 and 2"""
    rng = np.random.default_rng(seed)
    cfgs = [(n, 2), (n, 0), (n, 1)] if kind == 'quanonet' else [(n, 1), (n, 0), (n, 2)]
    blk = sum(ld for _, ld in cfgs)
    x = rng.uniform(-np.pi, np.pi, (2, n * len(cfgs)))
    w = rng.uniform(-np.pi, np.pi, (blk, 3, n))
    kw = dict(offset=0.3, coeff=1.7)
    if readout == 'diag':
        kw['ham_diag'] = rng.normal(size=1 << n)
    else:
        kw['ham_pauli'] = readout
    return cfgs, x, w, kw


@pytest.mark.parametrize('n', [2, 3, 4])
@pytest.mark.parametrize('readout', ['Z', 'X', 'Y', 'diag'])
def test_helper_walks_against_parameter_shift(n, readout):
    """the stored-state walk, the inverse walk and parameter shift through device_noise_reference.device_moments agree
    (n = 4, where the shift rule costs 96 evaluations of the literal reference per case: one model and idle setting per read-out)"""
    k = ('Z', 'X', 'Y', 'diag').index(readout)
    for kind in ('quanonet', 'heaqnn') if n < 4 else (('quanonet', 'heaqnn')[k % 2],):
        for idle in (True, False) if n < 4 else (k < 2,):
            cfgs, x, w, kw = _circuit_case(n, kind, readout, seed=10 * n + idle)
            nz = as_dict(device_noise(n, idle, seed=len(readout)), n)
            v0, gx0, gw0 = DV.circuit_grad(n, cfgs, x, w, nz, **kw)
            v1, gx1, gw1 = DV.circuit_grad(n, cfgs, x, w, nz, inverse=True, **kw)
            v2, gx2, gw2 = DV.shift_grad(n, cfgs, x, w, nz, **kw)
            err = max(np.abs(a - b).max() for a, b in ((v0, v2), (gx0, gx2), (gw0, gw2), (v1, v2), (gx1, gx2), (gw1, gw2)))
            print(f'n={n} {kind} {readout} idle={idle}: max|walk - shift|={err:.2e} max|g|={max(np.abs(gx2).max(), np.abs(gw2).max()):.2e}')
            assert err <= 1e-12
            assert max(np.abs(gx2).max(), np.abs(gw2).max()) > 1e-3              # not a vacuous comparison


def test_helper_relaxation_is_not_self_adjoint():
    """what the device walk adds to the uniform one: with b != 0 pulling O back through the channel itself (as the uniform
    walk may) gives another gradient than the Kraus adjoint"""
    n = 2
    cfgs, x, w, kw = _circuit_case(n, 'quanonet', 'Z', seed=1)
    nz = as_dict(device_noise(n, True, infinite_wire=None, scale=4.0), n)
    _, gx, gw = DV.shift_grad(n, cfgs, x, w, nz, **kw)
    saved = DV._kraus_on
    try:
        DV._kraus_on = lambda rho, n_, wires, kraus, adjoint=False: saved(rho, n_, wires, kraus)
        _, gx_self, gw_self = DV.circuit_grad(n, cfgs, x, w, nz, **kw)
    finally:
        DV._kraus_on = saved
    assert max(np.abs(gx - gx_self).max(), np.abs(gw - gw_self).max()) > 1e-3


@pytest.mark.parametrize('n', [2, 3, 4])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_helper_model_buffer(n, kind):
    """the whole [P + 2] buffer: circuit derivatives by parameter shift, the model around them by torch autograd"""
    from quanonet_amd.models import QuanONetPT
    rows = 3
    rng = np.random.default_rng(10 * n)
    combos = ((True, 'Z'), (False, 'X'), (True, 'Y'), (False, 'diag'))
    if n == 4:                                                           # the shift rule's cost again: two of the four
        combos = combos[:2] if kind == 'quanonet' else combos[2:]
    for trainable, readout in combos:
        if kind == 'quanonet':
            m = H.quanonet(n, 3, 2, (2, 0, 1, 2), n, if_trainable_freq=trainable, scale_coeff=0.7, ham_bound=(-2.0, 3.0),
                           **({'ham_diag': rng.normal(size=1 << n)} if readout == 'diag' else {'ham_pauli': readout}))
            ins = (torch.tensor(rng.uniform(-1, 1, (rows, 3))), torch.tensor(rng.uniform(0, 1, (rows, 2))))
        else:
            m = _model(kind, n, trainable, readout, seed=n)
            ins = (torch.tensor(rng.uniform(-1, 1, (rows, 4))),)
        y = rng.normal(size=rows)
        nz = as_dict(device_noise(n, trainable, seed=3), n)
        spec = DG.spec_of(m)
        flat = torch.cat([q.detach().reshape(-1) for q in m.parameters()]).numpy()
        trunk = ins[1].numpy() if len(ins) > 1 else None
        got, pred = DV.model_loss_grad(spec, flat, ins[0].numpy(), trunk, y, nz, 1.0 / 7)
        inv, _ = DV.model_loss_grad(spec, flat, ins[0].numpy(), trunk, y, nz, 1.0 / 7, inverse=True)
        if isinstance(m, QuanONetPT):
            x = torch.cat([m.trunk_freq(ins[1]), m.branch_freq(ins[0])], dim=1)
            cfgs, bias = O.block_configs_quanonet(n, m.net_size), m.bias
        else:
            x = m.freq(ins[0])
            cfgs, bias = O.block_configs_heaqnn(n, m.net_size), None
        qw = m.quantum_layer.ansatz_weights
        v, sx, sw = DV.shift_grad(n, cfgs, x.detach().numpy(), qw.detach().numpy(), nz, spec['offset'], spec['coeff'],
                                  spec['ham_diag'], spec['ham_pauli'])
        ref_pred = v + (float(bias.item()) if bias is not None else 0.0)
        np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=1e-12)
        g = torch.tensor(2.0 * (ref_pred - y) / 7)
        surrogate = (g[:, None] * torch.tensor(sx) * x).sum() + (torch.einsum('b,bskq->skq', g, torch.tensor(sw)) * qw).sum()
        if bias is not None:
            surrogate = surrogate + g.sum() * bias.sum()
        for q in m.parameters():
            q.grad = None
        surrogate.backward()
        ref = np.concatenate([(q.grad if q.grad is not None else torch.zeros_like(q)).reshape(-1).numpy() for q in m.parameters()]
                             + [np.array([((ref_pred - y) ** 2).sum(), (y ** 2).sum()])])
        assert got.shape == ref.shape
        print(f'n={n} {kind} {readout} trainable={trainable}: max|err|={np.abs(got - ref).max():.2e} max|g|={np.abs(ref).max():.2e}')
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(inv, ref, rtol=0, atol=1e-12)


def probe_setting(n, cfgs, target, idle=True):
    """(DeviceNoise, log10 A_dev) of the family device_noise(n, idle, scale=s) -- relaxation on every wire but one, so b != 0 --
    with s chosen for log10 A_dev = target"""
    if target == 0.0:
        from quanonet_amd.noise import DeviceNoise
        return DeviceNoise(), 0.0
    amp = lambda s: DV.log10_amplification(n, cfgs, as_dict(device_noise(n, idle, scale=s), n))
    lo, hi = 0.0, 1.0
    while amp(hi) < target:
        hi *= 2.0
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if amp(mid) < target else (lo, mid)
    return device_noise(n, idle, scale=lo), amp(lo)


PROBE_TARGETS = (0.0, 4.0, 7.0, 8.0, 11.99)            # scripts/device_noise_guard_probe.py adds 5 and 6


def probe(n, blocks, ld, targets=PROBE_TARGETS, seed=None):
    """[(log10 A_dev, max |inverse walk - stored walk| over value and gradients, max |gradient|)]"""
    rng = np.random.default_rng(n + blocks if seed is None else seed)
    cfgs = [(n, ld)] * blocks
    E, blk = n * blocks, blocks * ld
    x = rng.uniform(-np.pi, np.pi, (1, E))
    w = rng.uniform(-np.pi, np.pi, (blk, 3, n))
    out = []
    for target in targets:
        dn, logA = probe_setting(n, cfgs, target)
        assert abs(logA - target) < 1e-6
        nz = as_dict(dn, n)
        v0, gx0, gw0 = DV.circuit_grad(n, cfgs, x, w, nz, coeff=5.0 / n)
        v1, gx1, gw1 = DV.circuit_grad(n, cfgs, x, w, nz, coeff=5.0 / n, inverse=True)
        err = max(np.abs(gx0 - gx1).max(), np.abs(gw0 - gw1).max(), np.abs(v0 - v1).max())
        out.append((logA, err, max(np.abs(gx0).max(), np.abs(gw0).max())))
    return out


@pytest.mark.parametrize('n,blocks,ld', [(5, 30, 2), (5, 60, 2), (6, 10, 2)])
def test_conditioning_probe(n, blocks, ld):
    """
    The probe of test_noise_aware_abi.py under device settings with b != 0 (relaxation on every wire but one, idle decay on):
    the helper's inverse walk -- what the kernel does -- against its walk over stored forward states, on the same circuits
    (60 and 120 sub-layers at n = 5, 20 at n = 6).  The uniform walk's bound of 12 does not carry over: once b != 0 the
    observable no longer shrinks by what rho grows by, and the difference grows with A_dev.  Measured (largest of the three
    circuits): 6.1e-15 at log10 A_dev = 0, 2.1e-15 at 4, 1.3e-14 at 5, 4.5e-14 at 6, 2.4e-13 at 7, 1.5e-12 at 8, 1.1e-9 at
    11.99.  The criterion is the uniform walk's -- no probe at or below the bound above 1e-12 -- and 7 is the largest probed
    value that meets it; the settings above the bound are walked and printed, and the calls refuse them.  (5 and 6 are
    measured by scripts/device_noise_guard_probe.py, to keep this test short.)
    """
    for logA, err, gmax in probe(n, blocks, ld):
        inside = logA <= MAX_LOG10_AMPLIFICATION
        print(f'n={n} sub-layers={blocks * ld} log10A_dev={logA:.2f}: inverse walk - stored walk = {err:.2e}, max|g|={gmax:.2e}'
              + ('' if inside else '  (above the bound: refused)'))
        if inside:
            assert err <= 1e-12


def test_train_device_noise_parsing():
    from quanonet_amd import noise as N
    from quanonet_amd.solver import _train_device_noise, _train_noise
    dn = device_noise(3, True)
    assert _train_device_noise(None) is None
    assert _train_device_noise(dn) is dn
    assert _train_device_noise(dn.asdict()) == dn
    import json
    assert _train_device_noise(json.loads(json.dumps(dn.asdict(), allow_nan=False))) == dn
    for bad in (N.NoiseModel(p1=0.01), 0.1, 'dn', [0.1]):
        with pytest.raises(ValueError, match='train_device_noise'):
            _train_device_noise(bad)
    with pytest.raises((ValueError, TypeError)):
        _train_device_noise(N.NoiseModel(p1=0.01).asdict())                       # the other record's fields
    with pytest.raises(ValueError, match='train_noise and train_device_noise'):
        _train_device_noise(dn, train_noise=N.NoiseModel(p1=0.01))
    with pytest.raises(ValueError, match='train_noise and train_device_noise'):
        _train_device_noise(dn.asdict(), train_noise={'p1': 0.01})
    # the uniform calls still refuse a DeviceNoise, and say where it goes
    with pytest.raises(ValueError, match='DeviceNoise'):
        _train_noise(dn)
    m = H.heaqnn(2, 4, (3, 1), 0)
    with pytest.raises(ValueError, match='train_device_noise'):
        N.amplification(m, N.DeviceNoise())
    for call in (lambda: N.device_amplification(m, N.NoiseModel(p1=0.01)),
                 lambda: N.device_noisy_loss_and_grad(m, None, None, N.NoiseModel(p1=0.01))):
        with pytest.raises(ValueError, match='DeviceNoise'):
            call()
    # host only: the guard of a model under a setting
    assert N.device_amplification(m, N.DeviceNoise()) == 0.0
    assert abs(N.device_amplification(m, N.DeviceNoise.uniform(N.NoiseModel(p1=0.01, p2=0.02)))
               - N.amplification(m, N.NoiseModel(p1=0.01, p2=0.02))) <= 1e-12
    assert N.device_amplification(m, N.DeviceNoise(t1=1.0, t2=1.0, t_cx=0.1)) > 0.0
