"""
CPU checks of device-noise training from stored states (qhea_model_loss_grad_noisy_device_exact_stored /
qhea_model_train_steps_noisy_device_exact_stored): the symbols, the argument checks against their _device_exact twins (nothing
is launched, no GPU needed), the layer amplification against a numpy restatement, the workspace size (past 4 GiB too), every
refusal of the config key train_noise_states, and the condition on the inputs of tests/test_device_noise_stored_training.py:
past the bound the helper's inverse walk has left its stored walk while the gradient has not vanished.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import device_noise_grad_reference as DV
from tests.conftest import ROOT
from tests.test_device_noise_abi import BAD, _record
from tests.test_device_noise_training_abi import MAX_LOG10_AMPLIFICATION, _cfgs, _shapes, as_dict, device_noise, probe_setting

NEW = ('qhea_model_device_noisy_stored_grad_workspace_bytes', 'qhea_model_device_noisy_log10_layer_amplification',
       'qhea_model_loss_grad_noisy_device_exact_stored', 'qhea_model_train_steps_noisy_device_exact_stored')
PAST_THE_BOUND = ((3, (6, 2), 16.0, 3), (3, (6, 2), 20.0, 3), (5, (4, 2), 12.0, 1), (6, (3, 2), 12.0, 1))   # n, HEAQNN net, target, rows


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def _total(lib, d, rec):
    return lib.qhea_model_device_noisy_log10_amplification(ctypes.byref(d), ctypes.byref(rec))


def _layer(lib, d, rec):
    return lib.qhea_model_device_noisy_log10_layer_amplification(ctypes.byref(d), ctypes.byref(rec))


def _loss_grad(lib, d, batch, rec, stored=True, ham_diag=None):
    """the call with every array NULL: what the checks in front of the pointers return"""
    call = lib.qhea_model_loss_grad_noisy_device_exact_stored if stored else lib.qhea_model_loss_grad_noisy_device_exact
    return call(None if d is None else ctypes.byref(d), batch, None, None, None, None, ham_diag,
                None if rec is None else ctypes.byref(rec), 1.0, None, None, None, 0, None)


def _train_steps(lib, d, n_steps, rec, stored=True, first_step=1):
    call = lib.qhea_model_train_steps_noisy_device_exact_stored if stored else lib.qhea_model_train_steps_noisy_device_exact
    return call(None if d is None else ctypes.byref(d), n_steps, None, None, None, None, None, None,
                None if rec is None else ctypes.byref(rec), None, None, 0, None, None, first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                None, 0, None)


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 620 and _lib.MIN_LIB_VERSION >= 620
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    for f in (_lib.model_loss_grad_noisy_device_exact_stored, _lib.model_train_steps_noisy_device_exact_stored,
              _lib.model_device_noisy_log10_layer_amplification, _lib.model_device_noisy_stored_refused,
              _lib.model_device_noisy_stored_grad_workspace_bytes):
        assert callable(f)
    from quanonet_amd.noise import device_layer_amplification, device_noisy_loss_and_grad
    import inspect
    assert callable(device_layer_amplification)
    assert inspect.signature(device_noisy_loss_and_grad).parameters['states'].default == 'inverse'


def test_argument_checks_are_the_twins(lib):
    """every code of the _device_exact calls' argument checks, from the same calls in the same order"""
    from quanonet_amd import _lib
    n = 5
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    ok = _record(n)
    bad_desc = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    bad_desc.n_qubits = 0
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    dx = _lib.make_model_desc(_lib.MODEL_QUANONET, 3, (1, 1, 1, 1), 4, 1, True, 0.1, 0.0, 1.0)
    dx.ham_pauli = 1
    fake = ctypes.cast(ctypes.c_void_p(256), ctypes.POINTER(ctypes.c_double))
    for call in (_loss_grad, _train_steps):
        cases = [((bad_desc, 10, ok), -1), ((None, 10, ok), -1), ((d, 0, ok), 0), ((d, 10, None), -1), ((d, -1, ok), -1),
                 ((d7, 10, _record(7)), -2), ((d7, 10, _record(7, t_cx=-1.0)), -1), ((d7, 10, ok), -1), ((d, 10, ok), -1)]
        for over in BAD:
            cases += [((d, 10, _record(n, **over)), -1), ((d, 0, _record(n, **over)), -1)]
        for args, want in cases:
            assert call(lib, *args) == want == call(lib, *args, stored=False), (call.__name__, args[1], want)
    assert _train_steps(lib, d, 3, ok, first_step=0) == -1 == _train_steps(lib, d, 3, ok, stored=False, first_step=0)
    assert _loss_grad(lib, dx, 10, _record(3), ham_diag=fake) == -1 == _loss_grad(lib, dx, 10, _record(3), stored=False, ham_diag=fake)
    for f in (lib.qhea_model_device_noisy_stored_grad_workspace_bytes, lib.qhea_model_device_noisy_grad_workspace_bytes):
        assert f(ctypes.byref(d), -1) == 0 and f(None, 100) == 0 and f(ctypes.byref(bad_desc), 100) == 0


def test_train_steps_two_faults_at_once(lib):
    """the table of test_device_noise_training_abi.py: the stored call gives the twin's code for every pair of faults"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    from tests.test_noise_aware_abi import full_train_steps
    n = 5
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    d7 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 7, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    ok, bad = _record(n), _record(n, t_cx=-1.0)
    singular = DeviceNoise(p1=[0.01] * n, p2=[0.02] * n, t1=[1.0] * n, t2=[1.5] * n, t_rx=0.01, t_rot=0.02, t_cx=1e4).params(n)
    table = [('first_step 0, no row_begin', dict(d=d, nz=ok, first_step=0, row_begin=False), -1),
             ('first_step 0, invalid setting', dict(d=d, nz=bad, first_step=0), -1),
             ('first_step 0, n = 7', dict(d=d7, nz=_record(7), first_step=0), -2),
             ('first_step 0, singular site', dict(d=d, nz=singular, first_step=0), -2),
             ('first_step 0, no steps', dict(d=d, nz=ok, first_step=0, n_steps=0), -1),
             ('no steps alone', dict(d=d, nz=ok, n_steps=0), 0),
             ('no workspace, a valid call of two steps', dict(d=d, nz=ok), -3)]
    for what, kw, want in table:
        assert full_train_steps(lib, 'qhea_model_train_steps_noisy_device_exact_stored', **kw) == want, what
        assert full_train_steps(lib, 'qhea_model_train_steps_noisy_device_exact', **kw) == want, what


def _layer_reference(n, cfgs, dn):
    """numpy restatement: one sub-layer's ROT / CTL / TGT sites and CNOT slots, with the ENC sites if the circuit has encoding
    layers; the ENC sites alone for a circuit without sub-layers; inf where the total is"""
    nz = as_dict(dn, n)
    if any(p >= 0.75 for p in nz['p1']) or any(p >= 15.0 / 16.0 for p in nz['p2']):
        return math.inf
    chan, lam2 = dn.tables(n)
    blk = sum(ld for _, ld in cfgs)
    sites = ([0] if cfgs else []) + ([1, 2, 3] if blk else [])
    total = 0.0
    for k in sites:
        for q in range(n):
            m = min(chan[k][q][0], chan[k][q][1])
            if not m > 0.0:
                return math.inf
            total -= math.log10(m)
    if blk:
        total -= float(np.sum(np.log10(1.0 - np.asarray(lam2))))
    return total


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
def test_layer_amplification(lib, n):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    for seed, d in enumerate(_shapes(n)):
        for idle in (True, False):
            dn = device_noise(n, idle, seed=seed)
            rec = dn.params(n)
            got, total = _layer(lib, d, rec), _total(lib, d, rec)
            want = _layer_reference(n, _cfgs(d), dn)
            print(f'n={n} idle={idle} net={tuple(d.net)}: layer {got:.6f} (numpy {want:.6f}), total {total:.6f}')
            assert abs(got - want) <= 1e-12 and 0.0 < got <= total
    # a circuit of one unit: the layer is the circuit
    one = [_lib.make_model_desc(_lib.MODEL_HEAQNN, n, (1, 1), 4, 0, False, 0.1, 0.0, 1.0),
           _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (1, 0), 4, 0, True, 0.1, 0.0, 1.0)]
    for d in one:
        rec = device_noise(n, True, seed=4).params(n)
        assert _layer(lib, d, rec) == _total(lib, d, rec) > 0.0, tuple(d.net)
    # several units of one kind: the total is the count times the layer
    d = _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (5, 1), 4, 0, False, 0.1, 0.0, 1.0)
    rec = device_noise(n, True, seed=5).params(n)
    assert abs(5.0 * _layer(lib, d, rec) - _total(lib, d, rec)) <= 1e-12
    # +inf and NaN where the total is
    d = _shapes(n)[0]
    ok = dict(p1=[0.01] * n, p2=[0.02] * n, t1=[1.0] * n, t2=[1.5] * n, t_rx=0.01, t_rot=0.02, t_cx=0.03)
    for over in (dict(p1=[0.75] + [0.01] * (n - 1)), dict(p2=[0.02] * (n - 1) + [15 / 16]), dict(t_cx=1e4), dict(p1=[1.0] * n),
                 dict(t_rx=1e4), dict(t_rot=1e4)):
        rec = DeviceNoise(**dict(ok, **over)).params(n)
        assert _total(lib, d, rec) == math.inf and _layer(lib, d, rec) == math.inf, over
        assert _loss_grad(lib, d, 0, rec) == -2 and _train_steps(lib, d, 0, rec) == -2, over
    enc_only = one[1]                                                    # a site the circuit does not apply is not counted
    rec = DeviceNoise(**dict(ok, t_cx=1e4)).params(n)
    assert math.isfinite(_total(lib, enc_only, rec)) and _layer(lib, enc_only, rec) == _total(lib, enc_only, rec)
    bad_desc = _shapes(n)[0]
    bad_desc.n_qubits = 0
    assert math.isnan(_layer(lib, bad_desc, DeviceNoise(**ok).params(n))) and math.isnan(_total(lib, bad_desc, DeviceNoise(**ok).params(n)))
    assert math.isnan(_layer(lib, d, DeviceNoise().params(n + 1)))
    assert math.isnan(_layer(lib, d, _record(n, t_cx=-1.0)))
    assert math.isnan(lib.qhea_model_device_noisy_log10_layer_amplification(ctypes.byref(d), None))
    assert math.isnan(lib.qhea_model_device_noisy_log10_layer_amplification(None, ctypes.byref(DeviceNoise().params(n))))
    assert _layer(lib, d, DeviceNoise().params(n)) == 0.0


def test_the_guard_is_the_layer(lib):
    """the total is no reason to refuse; a layer above the inverse walk's bound is"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    n = 4
    d = _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (30, 2), 4, 0, False, 0.1, 0.0, 1.0)
    ok = dict(p1=[0.01] * n, p2=[0.02] * n, t1=[1.0] * n, t2=[1.5] * n, t_rx=0.01, t_rot=0.02, t_cx=0.03)
    rec = DeviceNoise(**ok).params(n)
    assert _total(lib, d, rec) > 2 * MAX_LOG10_AMPLIFICATION > MAX_LOG10_AMPLIFICATION > _layer(lib, d, rec)
    assert _loss_grad(lib, d, 0, rec, stored=False) == -2 and _train_steps(lib, d, 0, rec, stored=False) == -2
    assert _loss_grad(lib, d, 0, rec) == 0 and _train_steps(lib, d, 0, rec) == 0 and _loss_grad(lib, d, 10, rec) == -1
    assert _lib.model_device_noisy_refused(d, rec) and not _lib.model_device_noisy_stored_refused(d, rec)
    lo, hi = 0.0, 100.0                                                  # a long t_cx trips the layer bound without a singular site
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _layer(lib, d, DeviceNoise(**dict(ok, t_cx=mid)).params(n)) < MAX_LOG10_AMPLIFICATION else (lo, mid)
    above, below = DeviceNoise(**dict(ok, t_cx=hi * 1.001)).params(n), DeviceNoise(**dict(ok, t_cx=lo * 0.999)).params(n)
    assert MAX_LOG10_AMPLIFICATION < _layer(lib, d, above) < MAX_LOG10_AMPLIFICATION + 0.05
    assert MAX_LOG10_AMPLIFICATION - 0.05 < _layer(lib, d, below) < MAX_LOG10_AMPLIFICATION
    assert _loss_grad(lib, d, 0, above) == -2 and _train_steps(lib, d, 0, above) == -2 and _loss_grad(lib, d, 10, above) == -2
    assert _loss_grad(lib, d, 0, below) == 0 and _train_steps(lib, d, 0, below) == 0 and _loss_grad(lib, d, 10, below) == -1
    assert _lib.model_device_noisy_stored_refused(d, above) and not _lib.model_device_noisy_stored_refused(d, below)


def _align256(x):
    return (x + 255) // 256 * 256


def test_workspace_bytes(lib):
    from quanonet_amd import _lib
    inverse, stored = lib.qhea_model_device_noisy_grad_workspace_bytes, lib.qhea_model_device_noisy_stored_grad_workspace_bytes
    for n in (2, 3, 4, 5, 6):
        for d in _shapes(n):
            units = sum(max(ld, 1) for _, ld in _cfgs(d))
            for batch in (0, 1, 37, 100, 1000):
                want = inverse(ctypes.byref(d), batch) + _align256(units * batch * 16 * 4 ** n)
                assert stored(ctypes.byref(d), batch) == want, (n, tuple(d.net), batch)
                assert _lib.model_device_noisy_stored_grad_workspace_bytes(d, batch) == want
    # (2, 0, 1, 2): two encoding-only units and two sub-layers
    assert sum(max(ld, 1) for _, ld in _cfgs(_shapes(3)[2])) == 4
    # past 4 GiB: Q6 with 20 units at 3300 rows (the case of the GPU test), and the headline model at batch 1000
    d = _lib.make_model_desc(_lib.MODEL_HEAQNN, 6, (10, 2), 4, 0, False, 0.1, 0.0, 1.0)
    snap = 20 * 3300 * 16 * 4 ** 6
    assert snap > 1 << 32 and stored(ctypes.byref(d), 3300) == inverse(ctypes.byref(d), 3300) + _align256(snap)
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, 5, (40, 2, 20, 2), 100, 2, True, 0.1, 0.0, 1.0)
    assert stored(ctypes.byref(d), 1000) == inverse(ctypes.byref(d), 1000) + _align256(120 * 1000 * 16 * 4 ** 5)


def test_train_noise_states_parsing():
    from quanonet_amd import noise as N
    from quanonet_amd.solver import _train_noise_states
    dn, nm, sp = device_noise(3, True), N.NoiseModel(p1=0.01), N.Sampling(trajectories=8)
    assert _train_noise_states(None) == 'inverse' and _train_noise_states('inverse') == 'inverse'
    assert _train_noise_states('inverse', train_noise=nm) == 'inverse'                    # today's behaviour, whatever is beside it
    assert _train_noise_states(None, train_device_noise=dn, sampling_keys=['train_trajectories']) == 'inverse'
    assert _train_noise_states('stored', train_device_noise=dn) == 'stored'
    with pytest.raises(ValueError, match="train_noise_states='stored' does not combine with train_noise: under a uniform NoiseModel "
                                         "every gradient entry shrinks"):
        _train_noise_states('stored', train_noise=nm)
    for key in ('train_sampling', 'train_trajectories', 'train_jump_trajectories'):
        with pytest.raises(ValueError, match=f"train_noise_states='stored' does not combine with {key}: a sampled-trajectory "
                                             "gradient walks pure states"):
            _train_noise_states('stored', train_device_noise=dn, sampling_keys=[key])
    with pytest.raises(ValueError, match="train_noise_states='stored' needs train_device_noise"):
        _train_noise_states('stored')
    for bad in ('Stored', 'checkpoint', 1, True, ['stored']):
        with pytest.raises(ValueError, match="train_noise_states must be 'inverse' .* or 'stored'"):
            _train_noise_states(bad, train_device_noise=dn)
    # the trainer reads the key before it looks at the model: the same refusals from its constructor
    from quanonet_amd.solver import DataParallelTrainer
    for kw, text in ((dict(train_noise=nm), 'does not combine with train_noise'),
                     (dict(train_noise=nm, train_sampling=sp), 'does not combine with train_noise'),
                     (dict(train_device_noise=dn, train_sampling=sp), 'does not combine with train_sampling'),
                     (dict(train_device_noise=dn, train_trajectories=sp), 'does not combine with train_trajectories'),
                     (dict(train_device_noise=dn, train_jump_trajectories=sp), 'does not combine with train_jump_trajectories'),
                     (dict(), 'needs train_device_noise')):
        with pytest.raises(ValueError, match=text):
            DataParallelTrainer(None, train_noise_states='stored', **kw)
    with pytest.raises(ValueError, match='train_noise_states must be'):
        DataParallelTrainer(None, train_device_noise=dn, train_noise_states='snapshots')
    with pytest.raises(ValueError, match="states must be 'inverse' or 'stored'"):
        N.device_noisy_loss_and_grad(None, None, None, dn, states='kept')
    from tests import helpers as H
    m = H.heaqnn(2, 4, (3, 1), 0)
    with pytest.raises(ValueError, match='DeviceNoise'):
        N.device_layer_amplification(m, nm)
    assert N.device_layer_amplification(m, N.DeviceNoise()) == 0.0
    one = N.DeviceNoise(t1=1.0, t2=1.0, t_cx=0.1)
    assert 0.0 < N.device_layer_amplification(m, one) < N.device_amplification(m, one)


@pytest.mark.parametrize('n,net,target,rows', PAST_THE_BOUND)
def test_inputs_past_the_bound_are_not_vacuous(n, net, target, rows):
    """
    The condition on the inputs of test_past_the_bound (tests/test_device_noise_stored_training.py), on the CPU with the numpy
    helper: the largest gradient entry is >= 1e-3 at every setting (the GPU test does not pass on zeros), and at n = 3, targets
    16 and 20, the helper's inverse walk differs from its stored walk by > 1e-6 (the GPU test tells the two walks apart).
    The two settings at target 12 (n = 5 and n = 6, there for the indexing at those sizes where the inverse call refuses)
    cannot meet 1e-6: the drift grows about tenfold per unit of log10 A_dev and has only reached 1.3e-9 and 2.6e-10 there, so
    for them the difference is held above the GPU test's own tolerance, 1e-10.
    Measured (difference, largest entry): n = 3: 2.7e-4, 8.7e-3 at 16 and 0.30, 2.5e-3 at 20; n = 5: 1.3e-9, 7.4e-2; n = 6:
    2.6e-10, 3.2e-2.
    """
    from tests.test_device_noise_stored_training import ATOL, past_the_bound_case
    spec, flat, x, y, dn, logA = past_the_bound_case(n, net, target, rows)
    assert abs(logA - target) < 1e-6
    nz = as_dict(dn, n)
    stored, _ = DV.model_loss_grad(spec, flat, x, None, y, nz, 1.0 / rows)
    inverse, _ = DV.model_loss_grad(spec, flat, x, None, y, nz, 1.0 / rows, inverse=True)
    diff, gmax = np.abs(stored - inverse).max(), np.abs(stored[:-2]).max()
    print(f'n={n} net={net} log10 A_dev={logA:.2f}: |inverse walk - stored walk|={diff:.2e}, max|gradient|={gmax:.2e}')
    assert gmax >= 1e-3
    assert diff > (1e-6 if target >= 16.0 else ATOL)
