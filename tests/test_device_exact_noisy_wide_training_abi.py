"""
CPU checks of exact device-noise training at n = 7..9 (qhea_model_loss_grad_noisy_device_exact_wide /
qhea_model_train_steps_noisy_device_exact_wide): the symbols, the workspace layout restated in numpy, every return code that
comes back before a launch in device_call_check's order, the guard at its bound, log10 A_dev against the numpy helper at the new
sizes, the helper tests/device_noise_grad_reference.py at n = 7 against parameter shift, the conditioning probe that carries the
bound of 7 to n = 7 and 8, the table of [stage][local wire] records restated in numpy, and the parsing of the config key
train_device_noise_exact.  Nothing is launched.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import device_noise_grad_reference as DV
from tests import device_noise_reference as DNR
from tests.test_device_noise_abi import _record
from tests.test_device_noise_training_abi import (MAX_LOG10_AMPLIFICATION, _amp, _cfgs, as_dict, device_noise, probe,
                                                   probe_setting)
from tests.test_exact_noisy_wide import _pass_wires
from tests.test_exact_noisy_wide_training_abi import INT_MAX, _a256, _desc, _formula

NEW = ('qhea_model_device_noisy_wide_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_device_exact_wide',
       'qhea_model_train_steps_noisy_device_exact_wide')
TAB_WIRE = 66                            # kTabWire: [site][forward, inverse, adjoint][5], the slot's four factors, two readout rates
TABLE_BYTES = _a256(2 * 6 * TAB_WIRE * 8)


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    return _lib.load()


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 660 and _lib.MIN_LIB_VERSION >= 660
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert 'noisy_device_exact_wide' in _lib._GRAD_UNITS
    for f in (_lib.model_loss_grad_noisy_device_exact_wide, _lib.model_train_steps_noisy_device_exact_wide,
              _lib.model_device_noisy_wide_grad_workspace_bytes, _lib.model_device_noisy_wide_refused):
        assert callable(f)
    from quanonet_amd.noise import device_exact_noisy_loss_and_grad
    assert callable(device_exact_noisy_loss_and_grad)
    with pytest.raises(_lib.Unsupported, match='7..9'):                  # the unit's message for QHEA_EUNSUPPORTED names the range
        _lib._GRAD_UNITS['noisy_device_exact_wide'].check(-2, 'qhea_model_loss_grad_noisy_device_exact_wide', None, {})


def test_workspace_bytes(lib):
    """the uniform tiled unit's layout (prep tables | pred | records | h', h'^2 | partials | rho | O) with the table behind it,
    every region rounded up to 256 bytes"""
    size = lib.qhea_model_device_noisy_wide_grad_workspace_bytes
    for n in (2, 6, 10, 12):
        assert size(ctypes.byref(_desc(n)), 100) == 0
        assert size(ctypes.byref(_desc(n, 'heaqnn', (2, 1))), 100) == 0
    assert size(None, 100) == 0
    bad = _desc(7)
    bad.n_qubits = 0
    assert size(ctypes.byref(bad), 100) == 0
    for n in (7, 8, 9):
        for d, E, blk in ((_desc(n), 4 * n, 4), (_desc(n, 'heaqnn', (3, 0)), 3 * n, 0), (_desc(n, 'quanonet', (20, 2, 10, 2)), 30 * n, 60)):
            assert size(ctypes.byref(d), -1) == 0
            for B in (1, 100):
                got = size(ctypes.byref(d), B)
                assert got == _formula(lib, d, n, E, blk, B) + TABLE_BYTES, (n, E, blk, B)
                assert got == lib.qhea_model_exact_noisy_wide_grad_workspace_bytes(ctypes.byref(d), B) + TABLE_BYTES
        # no overflow at the largest batch the grid admits: the two matrices alone are 2 x 16 x 4^n bytes per row
        limit = INT_MAX >> (2 * (n - 6))
        d = _desc(n, 'quanonet', (20, 2, 10, 2))
        got = size(ctypes.byref(d), limit)
        assert got == _formula(lib, d, n, 30 * n, 60, limit) + TABLE_BYTES and got > 2 * 16 * limit * 4 ** n > 2 ** 44


def _loss_grad(lib, d, batch, rec, ham_diag=None, ws=None, ws_bytes=0, arrays=False):
    """the call with every array NULL (or, with `arrays`, a pointer nothing reads before the checks are through)"""
    p = ctypes.cast(ctypes.c_void_p(4096), ctypes.POINTER(ctypes.c_double)) if arrays else None
    return lib.qhea_model_loss_grad_noisy_device_exact_wide(None if d is None else ctypes.byref(d), batch, p, p, p, p, ham_diag,
                                                            None if rec is None else ctypes.byref(rec), 1.0, p, None, ws,
                                                            ws_bytes, None)


def _train_steps(lib, d, n_steps, rec, first_step=1):
    return lib.qhea_model_train_steps_noisy_device_exact_wide(None if d is None else ctypes.byref(d), n_steps, None, None, None,
                                                              None, None, None, None if rec is None else ctypes.byref(rec), None,
                                                              None, 0, None, None, first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0, None,
                                                              0, None)


def _full_train_steps(lib, d, nz, n_steps=2, first_step=1, row_begin=(0, 3, 5), ws=None, ws_bytes=0):
    """every array present (host memory: the checks read row_begin and nothing else); without a workspace nothing is launched"""
    from quanonet_amd import _lib
    P = _lib.model_param_count(d)
    buf = lambda k: (ctypes.c_double * k)()
    rb = (ctypes.c_int64 * 3)(*row_begin) if row_begin is not None else None
    return lib.qhea_model_train_steps_noisy_device_exact_wide(ctypes.byref(d), n_steps, rb, buf(64), buf(64), buf(8), buf(P), None,
                                                              ctypes.byref(nz), buf(2), buf(2 * (P + 2)), P + 2, buf(P), buf(P),
                                                              first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0, ws, ws_bytes, None)


def _bad_settings(n):
    """a QHEA_EINVAL setting of every kind device_noise_check knows, for n wires"""
    g = lambda v, bad, at=1: [bad if q == at else v for q in range(n)]
    return [dict(p1=None), dict(t2=None), dict(readout10=None), dict(n_wires=n - 1), dict(n_wires=0),
            dict(p1=g(0.01, -0.1)), dict(p2=g(0.01, 1.01, n - 1)), dict(readout01=g(0.01, 2.0)),
            dict(readout10=g(0.01, float('nan'), 0)), dict(t_rx=-1e-9), dict(t_rot=float('nan')), dict(t_cx=-0.5),
            dict(t1=g(1.0, 0.0)), dict(t2=g(1.0, -2.0, n - 1)), dict(t2=g(1.5, 2.0 + 1e-9, n - 1)),
            dict(t1=[1.0] * n, t2=g(1.0, math.inf))]


def test_return_codes_without_gpu(lib):
    """device_call_check's order: the descriptor, the setting's QHEA_EINVAL cases, the qubit range and the guard
    (QHEA_EUNSUPPORTED), the read-out, a negative count, the empty call, the NULL arrays; then the grid limit, then the workspace"""
    fake_ws = ctypes.c_void_p(1 << 20)                                   # never dereferenced: every call below returns first
    for n in (7, 8, 9):
        d = _desc(n)
        ok = _record(n)
        bad_desc = _desc(n)
        bad_desc.n_qubits = 0
        for call in (_loss_grad, _train_steps):
            assert call(lib, bad_desc, 10, ok) == -1
            assert call(lib, None, 10, ok) == -1
            assert call(lib, d, 0, ok) == 0                                       # empty batch / no steps
            assert call(lib, d, 10, None) == -1                                   # no setting
            for over in _bad_settings(n):
                assert call(lib, d, 10, _record(n, **over)) == -1, over
                assert call(lib, d, 0, _record(n, **over)) == -1, over            # ... before the empty batch is looked at
            assert call(lib, d, -1, ok) == -1
            assert call(lib, d, 10, _record(n - 1)) == -1                         # n - 1 wires for n qubits
            assert call(lib, d, 10, ok) == -1                                     # valid up to the NULL arrays
        assert _train_steps(lib, d, 3, ok, first_step=0) == -1
        # QHEA_EINVAL for a grid past 2^31 - 1 workgroups comes before QHEA_EWORKSPACE; one row fewer reaches the workspace check
        limit = INT_MAX >> (2 * (n - 6))
        assert _loss_grad(lib, d, limit + 1, ok, arrays=True) == -1
        assert _loss_grad(lib, d, limit + 1, ok, ws=fake_ws, ws_bytes=2 ** 63, arrays=True) == -1
        assert _loss_grad(lib, d, limit, ok, arrays=True) == -3
        need = lib.qhea_model_device_noisy_wide_grad_workspace_bytes(ctypes.byref(d), 10)
        assert _loss_grad(lib, d, 10, ok, arrays=True) == -3
        assert _loss_grad(lib, d, 10, ok, ws=fake_ws, ws_bytes=need - 1, arrays=True) == -3
        assert _full_train_steps(lib, d, ok) == -3
        need = lib.qhea_model_device_noisy_wide_grad_workspace_bytes(ctypes.byref(d), 3)       # the largest step has 3 rows
        assert _full_train_steps(lib, d, ok, ws=fake_ws, ws_bytes=need - 1) == -3
        assert _full_train_steps(lib, d, ok, row_begin=(0, limit + 1, limit + 2)) == -1
        # X / Y read-outs do not combine with ham_diag (as in every other call); the setting and the guard come first
        dx = _desc(n)
        dx.ham_pauli = 1
        diag = ctypes.cast(ctypes.c_void_p(256), ctypes.POINTER(ctypes.c_double))
        assert _loss_grad(lib, dx, 10, ok, ham_diag=diag) == -1
        assert _loss_grad(lib, dx, 10, _record(n, t_cx=1e4), ham_diag=diag) == -2
    for n in (2, 6, 10, 12):
        for d in (_desc(n), _desc(n, 'heaqnn', (2, 1))):
            for call in (_loss_grad, _train_steps):
                assert call(lib, d, 10, _record(n)) == -2
                assert call(lib, d, 0, _record(n)) == -2                          # ... before the empty batch is looked at
                assert call(lib, d, 10, _record(n, t_cx=-1.0)) == -1              # a bad setting is reported before the qubit count


def test_train_steps_two_faults_at_once(lib):
    """which code wins: as in the n <= 6 device unit (and unlike the uniform tiled unit) first_step = 0 is reported after the
    setting, the qubit range, the guard and the shared checks, and before the return of a call without steps"""
    d, d6, d10 = _desc(8), _desc(6), _desc(10)
    ok, bad, singular = _record(8), _record(8, t_cx=-1.0), _record(8, t_cx=1e4)
    table = [('first_step 0, no row_begin', dict(d=d, nz=ok, first_step=0, row_begin=None), -1),
             ('first_step 0, invalid setting', dict(d=d, nz=bad, first_step=0), -1),
             ('first_step 0, n = 6', dict(d=d6, nz=_record(6), first_step=0), -2),
             ('first_step 0, n = 10', dict(d=d10, nz=_record(10), first_step=0), -2),
             ('first_step 0, refused amplification', dict(d=d, nz=singular, first_step=0), -2),
             ('first_step 0, no steps', dict(d=d, nz=ok, first_step=0, n_steps=0), -1),
             ('no steps alone', dict(d=d, nz=ok, n_steps=0), 0),
             ('invalid setting, n = 10', dict(d=d10, nz=_record(10, t_cx=-1.0)), -1),
             ('n = 6, refused amplification', dict(d=d6, nz=_record(6, t_cx=1e4)), -2),
             ('refused amplification, no workspace', dict(d=d, nz=singular), -2),
             ('descending row_begin, no workspace', dict(d=d, nz=ok, row_begin=(0, 4, 2)), -1),
             ('no workspace, a valid call of two steps', dict(d=d, nz=ok), -3)]
    for what, kw, want in table:
        assert _full_train_steps(lib, **kw) == want, what


@pytest.mark.parametrize('n', [7, 8, 9])
def test_guard(lib, n):
    """7k's guard at the new sizes: log10 A_dev = 6.99 passes every check, 7.01 is refused before the empty batch is looked at,
    a singular channel is +inf"""
    from quanonet_amd.noise import DeviceNoise
    d = _desc(n, 'heaqnn', (10, 2))
    cfgs = _cfgs(d)
    for target, refused in ((6.99, False), (7.01, True)):
        dn, logA = probe_setting(n, cfgs, target)
        rec = dn.params(n)
        got = _amp(lib, d, rec)
        print(f'n={n}: target {target}, helper {logA:.6f}, library {got:.6f}')
        assert abs(got - target) < 1e-6 and (got > MAX_LOG10_AMPLIFICATION) == refused
        if refused:
            assert _loss_grad(lib, d, 0, rec) == -2 and _train_steps(lib, d, 0, rec) == -2
            assert _loss_grad(lib, d, 10, rec, arrays=True) == -2
        else:
            assert _loss_grad(lib, d, 0, rec) == 0 and _train_steps(lib, d, 0, rec) == 0
            assert _loss_grad(lib, d, 10, rec) == -1                              # reaches the NULL arrays
            assert _loss_grad(lib, d, 10, rec, arrays=True) == -3                 # ... and with them the workspace check
    ok = dict(p1=[0.001] * n, p2=[0.002] * n, t1=[1.0] * n, t2=[1.5] * n, t_rx=0.001, t_rot=0.002, t_cx=0.003)
    assert 0.0 < _amp(lib, d, DeviceNoise(**ok).params(n)) < MAX_LOG10_AMPLIFICATION
    for over in (dict(p1=[0.001] * (n - 1) + [0.75]), dict(p2=[15 / 16] + [0.002] * (n - 1)), dict(t_cx=1e4), dict(p1=[1.0] * n)):
        rec = DeviceNoise(**dict(ok, **over)).params(n)
        assert _amp(lib, d, rec) == math.inf, over
        assert _loss_grad(lib, d, 0, rec) == -2 and _train_steps(lib, d, 0, rec) == -2, over


@pytest.mark.parametrize('n', [7, 8, 9])
def test_amplification_at_the_new_sizes(lib, n):
    """qhea_model_device_noisy_log10_amplification answers at n = 7..9: the helper's value, and the uniform guard's for a
    uniform setting"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise, NoiseModel
    shapes = [_lib.make_model_desc(_lib.MODEL_QUANONET, n, (3, 2, 2, 1), 4, 1, True, 0.1, 0.0, 1.0),
              _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (4, 3), 4, 0, False, 0.1, 0.0, 1.0),
              _lib.make_model_desc(_lib.MODEL_QUANONET, n, (2, 0, 1, 2), 4, 1, True, 0.1, 0.0, 1.0)]
    for seed, d in enumerate(shapes):
        for idle in (True, False):
            dn = device_noise(n, idle, seed=seed)
            got = _amp(lib, d, dn.params(n))
            want = DV.log10_amplification(n, _cfgs(d), as_dict(dn, n))
            from_tables = DV.log10_amplification(n, _cfgs(d), as_dict(dn, n), tables=dn.tables(n))
            print(f'n={n} idle={idle} net={tuple(d.net)}: log10 A_dev={got:.6f} (helper {want:.6f})')
            assert abs(got - want) <= 1e-12 and abs(got - from_tables) <= 1e-12 and got > 0.0
        for p1, p2, ro in ((0.0, 0.0, 0.0), (1e-3, 1e-2, 1e-2), (0.03, 0.08, 0.04), (0.4, 0.0, 1.0)):
            nm = NoiseModel(p1=p1, p2=p2, readout=ro)
            want = lib.qhea_model_exact_noisy_log10_amplification(ctypes.byref(d), ctypes.byref(nm.params()))
            assert abs(_amp(lib, d, DeviceNoise.uniform(nm).params(n)) - want) <= 1e-12
    from tests import helpers as H
    from quanonet_amd.noise import device_amplification
    m = H.heaqnn(n, 4, (4, 3), 0)
    assert abs(device_amplification(m, device_noise(n, True)) - _amp(lib, shapes[1], device_noise(n, True).params(n))) <= 1e-12


# ---- the yardstick at the new size -----------------------------------------------------------------------------------------------

def test_helper_at_n7_against_parameter_shift():
    """
    DV.circuit_grad at n = 7, stored and inverse walk, against the two-term parameter-shift rule through the literal Kraus
    timeline (device_noise_reference.device_moments): the oracle of the GPU tests at the size they use it.  Blocks (7, 1),
    (7, 0).  One evaluation of the timeline costs a third of a second, so ten of the 35 angles are shifted: the three ansatz
    angles of the closing wire 6 and of wire 0, and the encoding angles of wires 0 and 6 in both blocks (columns 0, 6, 7, 13).
    """
    n, cfgs = 7, [(7, 1), (7, 0)]
    rng = np.random.default_rng(7)
    x = rng.uniform(-np.pi, np.pi, (2, 14))
    w = rng.uniform(-np.pi, np.pi, (1, 3, n))
    nz = as_dict(device_noise(n, True, seed=1), n)
    kw = dict(offset=0.3, coeff=0.7, ham_pauli='Y')
    f = lambda xx, ww: DNR.device_moments(n, cfgs, xx, ww, nz, kw['offset'], kw['coeff'], None, kw['ham_pauli'])[0]
    value = f(x, w)
    cols = (0, 6, 7, 13)
    angles = [(0, k, q) for q in (6, 0) for k in range(3)]
    sx, sw = {}, {}
    for e in cols:
        xp, xm = x.copy(), x.copy()
        xp[:, e] += np.pi / 2
        xm[:, e] -= np.pi / 2
        sx[e] = 0.5 * (f(xp, w) - f(xm, w))
    for idx in angles:
        wp, wm = w.copy(), w.copy()
        wp[idx] += np.pi / 2
        wm[idx] -= np.pi / 2
        sw[idx] = 0.5 * (f(x, wp) - f(x, wm))
    gmax = max(max(np.abs(v).max() for v in sx.values()), max(np.abs(v).max() for v in sw.values()))
    walks = {}
    for inverse in (False, True):
        v1, gx, gw = walks[inverse] = DV.circuit_grad(n, cfgs, x, w, nz, inverse=inverse, **kw)
        err = max([np.abs(v1 - value).max()] + [np.abs(gx[:, e] - sx[e]).max() for e in cols]
                  + [np.abs(gw[(slice(None),) + idx] - sw[idx]).max() for idx in angles])
        print(f'n=7 inverse={inverse}: max|err against parameter shift|={err:.2e} max|g|={gmax:.2e}')
        assert err <= 1e-12
    assert gmax > 1e-3                                                   # not a vacuous comparison
    diff = max(np.abs(a - b).max() for a, b in zip(walks[False], walks[True]))
    print(f'n=7 log10A_dev={DV.log10_amplification(n, cfgs, nz):.2f}: inverse walk - stored walk = {diff:.2e}')
    assert diff <= 1e-12


@pytest.mark.parametrize('n,blocks,ld', [(7, 10, 2), (8, 5, 2)])
def test_conditioning_probe(n, blocks, ld):
    """
    The probe that fixed the bound of 7 at n <= 6 (tests/test_device_noise_training_abi.py), at the new sizes: the helper's
    inverse walk -- what the kernels do -- against its walk over stored forward states under settings with relaxation on every
    wire but one.  Measured: n = 7 with 20 sub-layers 1.1e-15 at log10 A_dev = 0, 1.2e-16 at 4, 9.8e-15 at 7, 6.7e-14 at 8;
    n = 8 with 10 sub-layers 5.3e-16, 6.1e-17, 6.2e-15, 3.1e-14.  The criterion is that of the bound -- no probe at or below
    it above 1e-12 -- so 7 carries over; 8 is walked and printed, and the calls refuse it.
    """
    for logA, err, gmax in probe(n, blocks, ld, targets=(0.0, 4.0, 7.0, 8.0)):
        inside = logA <= MAX_LOG10_AMPLIFICATION
        print(f'n={n} sub-layers={blocks * ld} log10A_dev={logA:.2f}: inverse walk - stored walk = {err:.2e}, max|g|={gmax:.2e}'
              + ('' if inside else '  (above the bound: refused)'))
        if inside:
            assert err <= 1e-12


# ---- the table ---------------------------------------------------------------------------------------------------------------------

def _global_wire(n, stage, local):
    """global_wire<N, STAGE> of hea_density_device_wide_stages.hpp"""
    return local if stage == 0 or local < 2 else local + n - 6


def _table_reads(n):
    """
    What the reverse stages read of the table of [stage][local wire] records, restated from the passes: per (stage, local
    wire, site) the global (wire, site) it must hold, and per (stage, local pass) the slot.  Reverse ring pass J runs on
    Pass<6, J < 5 ? J : J - n + 6> of stage A (J < 5) or B.
    """
    ENC, ROT, CTL, TGT = range(4)
    sites, slots = {}, {}

    def read(stage, local, site, wire):
        assert (stage, local, site) not in sites, (stage, local, site)
        sites[stage, local, site] = (wire, site)

    for J in range(n - 1, -1, -1):
        stage, LJ = (0, J) if J < 5 else (1, J - n + 6)
        assert 0 <= LJ <= 5
        t, c = _pass_wires(LJ)
        assert (_global_wire(n, stage, t), _global_wire(n, stage, c)) == (J, (J + 1) % n)
        read(stage, t, TGT, J)
        read(stage, c, CTL, (J + 1) % n)
        assert (stage, LJ) not in slots
        slots[stage, LJ] = J
        pending = ([(c, J + 1)] if J <= n - 2 else []) + ([(t, 0)] if J == 0 else [])
        for local, wire in pending:
            assert _global_wire(n, stage, local) == wire
            read(stage, local, ROT, wire)
            read(stage, local, ENC, wire)
    return sites, slots


@pytest.mark.parametrize('n', [7, 8, 9])
def test_stage_table(n):
    """every global wire's four sites and every slot appear exactly once across the two stages, at the local index the pass
    uses; the table kernel's placement (record [stage][l] = wire global_wire(stage, l), slot l or l + n - 6) serves every read;
    the encoding-only stages read the kEnc entries the ring stages read"""
    sites, slots = _table_reads(n)
    assert sorted(sites.values()) == [(q, s) for q in range(n) for s in range(4)]
    assert sorted(slots.values()) == list(range(n))
    for (stage, local, site), (wire, _) in sites.items():
        assert _global_wire(n, stage, local) == wire                     # what dev_wide_table_kernel puts there
    for (stage, LJ), slot in slots.items():
        assert (LJ if stage == 0 else LJ + n - 6) == slot
    assert slots[1, 5] == n - 1 and sites[1, 5, 3] == (n - 1, 3) and sites[1, 0, 2] == (0, 2)     # the closing pair (5, 0) of stage B
    # a block without sub-layers: stage B serves local wires >= 12 - n (global 6..n-1), stage A local 0..5
    enc = [(1, l) for l in range(12 - n, 6)] + [(0, l) for l in range(6)]
    assert sorted(_global_wire(n, s, l) for s, l in enc) == list(range(n))
    for s, l in enc:
        assert sites[s, l, 0] == (_global_wire(n, s, l), 0)


def test_table_forms():
    """the two forms of a site as the host composes them, against the Kraus channel: the inverse form undoes the forward
    form, the adjoint form is its transpose on the populations"""
    off, a, b = 0.9, 0.8, 0.15

    def element_form(off, a, b):
        return off, 0.5 * (1 + a + b), 0.5 * (1 - a + b), 0.5 * (1 - a - b), 0.5 * (1 + a - b)

    def apply(form, rho):
        o, k00, k01, k10, k11 = form
        return np.array([[k00 * rho[0, 0] + k01 * rho[1, 1], o * rho[0, 1]], [o * rho[1, 0], k10 * rho[0, 0] + k11 * rho[1, 1]]])

    fwd, inv = element_form(off, a, b), element_form(1 / off, 1 / a, -b / a)
    adj = (fwd[0], fwd[1], fwd[3], fwd[2], fwd[4])
    rng = np.random.default_rng(0)
    rho = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))
    obs = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))
    np.testing.assert_allclose(apply(inv, apply(fwd, rho)), rho, rtol=0, atol=1e-14)
    assert abs(np.trace(obs.conj().T @ apply(fwd, rho)) - np.trace(apply(adj, obs).conj().T @ rho)) < 1e-14


def test_train_device_noise_exact_parsing():
    from quanonet_amd.noise import NoiseModel, Sampling
    from quanonet_amd.solver import _train_device_noise_exact
    dn = device_noise(7, True)
    assert _train_device_noise_exact(None) is None and _train_device_noise_exact(None, dn, ['train_noise']) is None
    assert _train_device_noise_exact('wide', dn) == 'wide'
    with pytest.raises(ValueError, match="None or 'wide'"):
        _train_device_noise_exact('tiled', dn)
    with pytest.raises(ValueError, match='needs train_device_noise'):
        _train_device_noise_exact('wide')
    for key in ('train_noise', 'train_sampling', 'train_trajectories', 'train_jump_trajectories'):
        with pytest.raises(ValueError, match=key):
            _train_device_noise_exact('wide', dn, [key])
    from quanonet_amd.noise import device_exact_noisy_loss_and_grad
    from tests import helpers as H
    with pytest.raises(ValueError, match='wide_exact_noisy_loss_and_grad'):
        device_exact_noisy_loss_and_grad(H.heaqnn(7, 4, (1, 1), 0), None, None, NoiseModel(p1=0.01))
    with pytest.raises(ValueError, match='device_trajectory_loss_and_grad'):
        device_exact_noisy_loss_and_grad(H.heaqnn(10, 4, (1, 1), 0), None, None, dn)
    with pytest.raises(TypeError):
        import torch
        device_exact_noisy_loss_and_grad(torch.nn.Linear(2, 1), None, None, dn)
    assert Sampling is not None
