"""
CPU checks of exact device-noise training from stored states at n = 7..9 (qhea_model_loss_grad_noisy_device_exact_wide_stored /
qhea_model_train_steps_noisy_device_exact_wide_stored): the symbols and the version, the workspace restated in numpy (the
inverse unit's plus units x rows x 16 x 4^n, rounded up to 256) for the three table rows of
tests/test_device_exact_noisy_wide_training_abi.py, 0 outside n = 7..9, the refusals in their order (the qubit range, the layer
amplification in place of the total, a singular channel, first_step < 1 where the inverse unit reports it), that the settings
the GPU tests use past the bound are not vacuous (the helper's inverse walk there differs from its stored walk by more than
ten times the tolerance), and the parsing of the config value train_device_noise_exact='stored'.  Nothing is launched.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import device_noise_grad_reference as DV
from tests.test_device_noise_abi import _record
from tests.test_device_noise_training_abi import MAX_LOG10_AMPLIFICATION, _amp, _cfgs, as_dict, probe_setting
from tests.test_exact_noisy_wide_training_abi import INT_MAX, _a256, _desc

NEW = ('qhea_model_device_noisy_wide_stored_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_device_exact_wide_stored',
       'qhea_model_train_steps_noisy_device_exact_wide_stored')
ATOL = 1e-10
# (n, log10 A_dev) of the GPU test past the bound: a fixed-frequency HEAQNN (3, 2), one row
PAST_THE_BOUND = ((7, 16.0), (7, 20.0), (8, 16.0), (9, 16.0))
PAST_NET = (3, 2)


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    return _lib.load()


def _layer(lib, d, rec):
    return lib.qhea_model_device_noisy_log10_layer_amplification(ctypes.byref(d), ctypes.byref(rec))


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 670 and _lib.MIN_LIB_VERSION >= 670
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert 'noisy_device_exact_wide_stored' in _lib._GRAD_UNITS
    for f in (_lib.model_loss_grad_noisy_device_exact_wide_stored, _lib.model_train_steps_noisy_device_exact_wide_stored,
              _lib.model_device_noisy_wide_stored_grad_workspace_bytes, _lib.model_device_noisy_wide_stored_refused):
        assert callable(f)
    with pytest.raises(_lib.Unsupported, match='7..9'):                  # the unit's message for QHEA_EUNSUPPORTED names the range
        _lib._GRAD_UNITS['noisy_device_exact_wide_stored'].check(-2, 'qhea_model_loss_grad_noisy_device_exact_wide_stored', None, {})


def test_workspace_bytes(lib):
    """the inverse unit's workspace with the snapshot region behind it: U x B x 16 x 4^n bytes rounded up to 256, U = sub-layers
    + blocks without sub-layers"""
    from quanonet_amd import _lib
    size = lib.qhea_model_device_noisy_wide_stored_grad_workspace_bytes
    inverse = lib.qhea_model_device_noisy_wide_grad_workspace_bytes
    for n in (2, 6, 10, 12):
        assert size(ctypes.byref(_desc(n)), 100) == 0
        assert size(ctypes.byref(_desc(n, 'heaqnn', (2, 1))), 100) == 0
    assert size(None, 100) == 0
    bad = _desc(7)
    bad.n_qubits = 0
    assert size(ctypes.byref(bad), 100) == 0
    for n in (7, 8, 9):
        # QuanONet (2, 1, 2, 1): 4 units; HEAQNN (3, 0): three encoding-only units; Net20-2-10-2: 60 units
        for d, U in ((_desc(n), 4), (_desc(n, 'heaqnn', (3, 0)), 3), (_desc(n, 'quanonet', (20, 2, 10, 2)), 60)):
            assert size(ctypes.byref(d), -1) == 0
            for B in (1, 100):
                got = size(ctypes.byref(d), B)
                assert got == inverse(ctypes.byref(d), B) + _a256(U * B * 16 * 4 ** n), (n, U, B)
                assert _lib.model_device_noisy_wide_stored_grad_workspace_bytes(d, B) == got
                assert _lib.model_device_noisy_wide_stored_grad_workspace_bytes(d, B, snapshots_only=True) == U * B * 16 * 4 ** n
        # QuanONet (2, 0, 1, 2): a block of two sub-layers and two without any -- 4 units
        d = _desc(n, 'quanonet', (2, 0, 1, 2))
        assert size(ctypes.byref(d), 3) == inverse(ctypes.byref(d), 3) + 4 * 3 * 16 * 4 ** n
        # no overflow at the largest batch the grid admits
        limit = INT_MAX >> (2 * (n - 6))
        d = _desc(n, 'quanonet', (20, 2, 10, 2))
        got = size(ctypes.byref(d), limit)
        assert got == inverse(ctypes.byref(d), limit) + 60 * limit * 16 * 4 ** n and got > 2 ** 49
    # a circuit without blocks has no unit and no snapshot
    d = _desc(7, 'heaqnn', (0, 2))
    if inverse(ctypes.byref(d), 5):
        assert size(ctypes.byref(d), 5) == inverse(ctypes.byref(d), 5)


def _loss_grad(lib, d, batch, rec, ws=None, ws_bytes=0, arrays=False):
    p = ctypes.cast(ctypes.c_void_p(4096), ctypes.POINTER(ctypes.c_double)) if arrays else None
    return lib.qhea_model_loss_grad_noisy_device_exact_wide_stored(None if d is None else ctypes.byref(d), batch, p, p, p, p, None,
                                                                   None if rec is None else ctypes.byref(rec), 1.0, p, None, ws,
                                                                   ws_bytes, None)


def _inverse_loss_grad(lib, d, batch, rec):
    return lib.qhea_model_loss_grad_noisy_device_exact_wide(ctypes.byref(d), batch, None, None, None, None, None, ctypes.byref(rec),
                                                            1.0, None, None, None, 0, None)


def _train_steps(lib, d, n_steps, rec, first_step=1):
    return lib.qhea_model_train_steps_noisy_device_exact_wide_stored(None if d is None else ctypes.byref(d), n_steps, None, None,
                                                                     None, None, None, None,
                                                                     None if rec is None else ctypes.byref(rec), None, None, 0,
                                                                     None, None, first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, 0,
                                                                     None)


def _full_train_steps(lib, d, nz, n_steps=2, first_step=1, row_begin=(0, 3, 5), ws=None, ws_bytes=0):
    """every array present (host memory: the checks read row_begin and nothing else); without a workspace nothing is launched"""
    from quanonet_amd import _lib
    P = _lib.model_param_count(d)
    buf = lambda k: (ctypes.c_double * k)()
    rb = (ctypes.c_int64 * 3)(*row_begin) if row_begin is not None else None
    return lib.qhea_model_train_steps_noisy_device_exact_wide_stored(ctypes.byref(d), n_steps, rb, buf(64), buf(64), buf(8), buf(P),
                                                                     None, ctypes.byref(nz), buf(2), buf(2 * (P + 2)), P + 2, buf(P),
                                                                     buf(P), first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0, ws, ws_bytes,
                                                                     None)


def test_return_codes_without_gpu(lib):
    """the inverse unit's order with the layer amplification in the guard's place"""
    fake_ws = ctypes.c_void_p(1 << 20)                                   # never dereferenced: every call below returns first
    for n in (7, 8, 9):
        d, ok = _desc(n), _record(n)
        bad_desc = _desc(n)
        bad_desc.n_qubits = 0
        for call in (_loss_grad, _train_steps):
            assert call(lib, bad_desc, 10, ok) == -1
            assert call(lib, None, 10, ok) == -1
            assert call(lib, d, 0, ok) == 0                                       # empty batch / no steps
            assert call(lib, d, 10, None) == -1                                   # no setting
            assert call(lib, d, 10, _record(n, t_cx=-0.5)) == -1
            assert call(lib, d, 0, _record(n, t_cx=-0.5)) == -1                   # ... before the empty batch is looked at
            assert call(lib, d, -1, ok) == -1
            assert call(lib, d, 10, _record(n - 1)) == -1                         # n - 1 wires for n qubits
            assert call(lib, d, 10, ok) == -1                                     # valid up to the NULL arrays
        assert _train_steps(lib, d, 3, ok, first_step=0) == -1
        limit = INT_MAX >> (2 * (n - 6))
        assert _loss_grad(lib, d, limit + 1, ok, ws=fake_ws, ws_bytes=2 ** 63, arrays=True) == -1
        assert _loss_grad(lib, d, limit, ok, arrays=True) == -3
        need = lib.qhea_model_device_noisy_wide_stored_grad_workspace_bytes(ctypes.byref(d), 10)
        assert need > lib.qhea_model_device_noisy_wide_grad_workspace_bytes(ctypes.byref(d), 10)
        assert _loss_grad(lib, d, 10, ok, ws=fake_ws, ws_bytes=need - 1, arrays=True) == -3
        # a workspace that would do for the inverse call does not do here
        assert _loss_grad(lib, d, 10, ok, ws=fake_ws, ws_bytes=lib.qhea_model_device_noisy_wide_grad_workspace_bytes(
            ctypes.byref(d), 10), arrays=True) == -3
        assert _full_train_steps(lib, d, ok) == -3
        need = lib.qhea_model_device_noisy_wide_stored_grad_workspace_bytes(ctypes.byref(d), 3)    # the largest step has 3 rows
        assert _full_train_steps(lib, d, ok, ws=fake_ws, ws_bytes=need - 1) == -3
        assert _full_train_steps(lib, d, ok, row_begin=(0, limit + 1, limit + 2)) == -1
    for n in (2, 6, 10, 12):
        for d in (_desc(n), _desc(n, 'heaqnn', (2, 1))):
            for call in (_loss_grad, _train_steps):
                assert call(lib, d, 10, _record(n)) == -2
                assert call(lib, d, 0, _record(n)) == -2                          # ... before the empty batch is looked at
                assert call(lib, d, 10, _record(n, t_cx=-1.0)) == -1              # a bad setting is reported before the qubit count


def test_train_steps_two_faults_at_once(lib):
    """first_step = 0 is reported where the inverse unit reports it: after the setting, the qubit range, the guard and the shared
    checks, and before the return of a call without steps"""
    d, d6, d10 = _desc(8), _desc(6), _desc(10)
    ok, bad, singular = _record(8), _record(8, t_cx=-1.0), _record(8, t_cx=1e4)
    table = [('first_step 0, no row_begin', dict(d=d, nz=ok, first_step=0, row_begin=None), -1),
             ('first_step 0, invalid setting', dict(d=d, nz=bad, first_step=0), -1),
             ('first_step 0, n = 6', dict(d=d6, nz=_record(6), first_step=0), -2),
             ('first_step 0, n = 10', dict(d=d10, nz=_record(10), first_step=0), -2),
             ('first_step 0, singular channel', dict(d=d, nz=singular, first_step=0), -2),
             ('first_step 0, no steps', dict(d=d, nz=ok, first_step=0, n_steps=0), -1),
             ('no steps alone', dict(d=d, nz=ok, n_steps=0), 0),
             ('singular channel, no workspace', dict(d=d, nz=singular), -2),
             ('descending row_begin, no workspace', dict(d=d, nz=ok, row_begin=(0, 4, 2)), -1),
             ('no workspace, a valid call of two steps', dict(d=d, nz=ok), -3)]
    for what, kw, want in table:
        assert _full_train_steps(lib, **kw) == want, what


@pytest.mark.parametrize('n', [7, 8, 9])
def test_guard_is_the_layer_amplification(lib, n):
    """a total log10 A_dev of 16 on ten blocks of two sub-layers is refused by the inverse call and passes here, its layer
    value far below 7; a setting whose single layer passes 7 is refused before the empty batch is looked at; a singular channel
    is +inf"""
    from quanonet_amd.noise import DeviceNoise
    d = _desc(n, 'heaqnn', (10, 2))
    cfgs = _cfgs(d)
    dn, logA = probe_setting(n, cfgs, 16.0)
    rec = dn.params(n)
    layer = _layer(lib, d, rec)
    print(f'n={n}: total {_amp(lib, d, rec):.4f} (helper {logA:.4f}), layer {layer:.4f}')
    assert abs(_amp(lib, d, rec) - 16.0) < 1e-6 and 0.0 < layer <= MAX_LOG10_AMPLIFICATION
    assert _inverse_loss_grad(lib, d, 0, rec) == -2
    assert _loss_grad(lib, d, 0, rec) == 0 and _train_steps(lib, d, 0, rec) == 0
    assert _loss_grad(lib, d, 10, rec, arrays=True) == -3                     # through every check up to the workspace
    # one unit past the bound, no channel singular: p2 = 0.9 on every slot is -log10(1 - 16/15 x 0.9) = 1.40 per slot, n slots
    for p2, refused in ((0.5, False), (0.9, True)):
        rec1 = DeviceNoise(p2=[p2] * n).params(n)
        layer1 = _layer(lib, d, rec1)
        assert abs(layer1 + n * math.log10(1.0 - 16.0 / 15.0 * p2)) < 1e-9 and math.isfinite(layer1)
        assert (layer1 > MAX_LOG10_AMPLIFICATION) == refused
        want = -2 if refused else 0
        assert _loss_grad(lib, d, 0, rec1) == want and _train_steps(lib, d, 0, rec1) == want
        assert _loss_grad(lib, d, 10, rec1, arrays=True) == (-2 if refused else -3)
        # one block of one sub-layer is one unit: its total is its layer value
        d1 = _desc(n, 'heaqnn', (1, 1))
        assert abs(_amp(lib, d1, rec1) - _layer(lib, d1, rec1)) < 1e-12 and abs(_layer(lib, d1, rec1) - layer1) < 1e-12
    ok = dict(p1=[0.001] * n, p2=[0.002] * n, t1=[1.0] * n, t2=[1.5] * n, t_rx=0.001, t_rot=0.002, t_cx=0.003)
    for over in (dict(p1=[0.001] * (n - 1) + [0.75]), dict(p2=[15 / 16] + [0.002] * (n - 1)), dict(t_cx=1e4)):
        rec = DeviceNoise(**dict(ok, **over)).params(n)
        assert _layer(lib, d, rec) == math.inf, over
        assert _loss_grad(lib, d, 0, rec) == -2 and _train_steps(lib, d, 0, rec) == -2, over


@pytest.mark.parametrize('n,target', PAST_THE_BOUND)
def test_past_the_bound_settings_are_not_vacuous(n, target):
    """on the inputs of the GPU test past the bound the helper's inverse walk differs from its stored walk by more than 1e-9, ten
    times the tolerance: a kernel that walked rho back through the inverses would fail that test"""
    from tests.test_device_noise_stored_training import past_the_bound_case
    spec, flat, x, y, dn, logA = past_the_bound_case(n, PAST_NET, target, 1)
    assert abs(logA - target) < 1e-6
    nz = as_dict(dn, n)
    stored, _ = DV.model_loss_grad(spec, flat, x, None, y, nz, 1.0, inverse=False)
    inverse, _ = DV.model_loss_grad(spec, flat, x, None, y, nz, 1.0, inverse=True)
    diff = np.abs(stored - inverse).max()
    print(f'n={n} log10 A_dev={logA:.2f}: max|inverse walk - stored walk|={diff:.2e} max|gradient|={np.abs(stored[:-2]).max():.2e}')
    assert diff > 10 * ATOL
    assert np.abs(stored[:-2]).max() >= 1e-3


def test_train_device_noise_exact_stored_parsing():
    from quanonet_amd.noise import DeviceNoise
    from quanonet_amd.solver import _train_device_noise_exact
    dn = DeviceNoise(p1=0.01)
    assert _train_device_noise_exact('stored', dn) == 'stored'
    assert _train_device_noise_exact('stored', dn, (), 'stored') == 'stored'
    assert _train_device_noise_exact('wide', dn, (), 'stored') == 'wide'
    assert _train_device_noise_exact(None, None, ('train_noise',)) is None
    with pytest.raises(ValueError, match="None or 'wide'.*'stored'"):
        _train_device_noise_exact('snapshots', dn)
    with pytest.raises(ValueError, match="'stored' needs train_device_noise"):
        _train_device_noise_exact('stored', None)
    for key in ('train_noise', 'train_sampling', 'train_trajectories', 'train_jump_trajectories'):
        with pytest.raises(ValueError, match=f"'stored' does not combine with {key}"):
            _train_device_noise_exact('stored', dn, (key,))
    with pytest.raises(ValueError, match="absent or 'stored'"):
        _train_device_noise_exact('stored', dn, (), 'inverse')
