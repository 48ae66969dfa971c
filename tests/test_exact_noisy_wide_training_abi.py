"""
CPU checks of exact noise-aware training at n = 7..9 (qhea_model_loss_grad_noisy_exact_wide /
qhea_model_train_steps_noisy_exact_wide): the symbols, the workspace formula of the header, every return code that comes back
before a launch, the conditioning guard, the tile maps as the reverse stages use them (a trace is the sum of its tiles'
shares), and the numpy helper tests/density_grad_reference.py at n = 7 against parameter shift.  Nothing is launched.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import density_grad_reference as DG
from tests import density_reference as DR

NEW = ('qhea_model_exact_noisy_wide_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_exact_wide',
       'qhea_model_train_steps_noisy_exact_wide')
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    return _lib.load()


def _desc(n, model='quanonet', net=(2, 1, 2, 1)):
    from quanonet_amd import _lib
    if model == 'quanonet':
        return _lib.make_model_desc(_lib.MODEL_QUANONET, n, net, 4, 1, True, 0.1, 0.0, 1.0)
    return _lib.make_model_desc(_lib.MODEL_HEAQNN, n, net, 3, 0, False, 0.1, 0.0, 1.0)


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 650 and _lib.MIN_LIB_VERSION >= 650
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert 'noisy_exact_wide' in _lib._GRAD_UNITS
    for f in (_lib.model_loss_grad_noisy_exact_wide, _lib.model_train_steps_noisy_exact_wide,
              _lib.model_exact_noisy_wide_grad_workspace_bytes):
        assert callable(f)
    from quanonet_amd.noise import wide_exact_noisy_loss_and_grad
    assert callable(wide_exact_noisy_loss_and_grad)
    # the unit's message for QHEA_EUNSUPPORTED names the range
    with pytest.raises(_lib.Unsupported, match='7..9'):
        _lib._GRAD_UNITS['noisy_exact_wide'].check(-2, 'qhea_model_loss_grad_noisy_exact_wide', None, {})


def _a256(v):
    return (v + 255) // 256 * 256


def _formula(lib, d, n, E, blk, B):
    """the header's workspace formula: prep tables | pred | records | h', h'^2 | partials | rho | O, each rounded up to 256"""
    A = E + 3 * n * blk
    tables = lib.qhea_model_exact_noisy_workspace_bytes(ctypes.byref(d), B)
    return (tables + _a256(8 * B) + _a256(8 * A * B) + _a256(8 * 2 * 2 ** n) + _a256(8 * A * B * 4 ** (n - 6))
            + 2 * _a256(16 * B * 4 ** n))


def test_workspace_bytes(lib):
    size = lib.qhea_model_exact_noisy_wide_grad_workspace_bytes
    for n in (2, 6, 10, 12):
        assert size(ctypes.byref(_desc(n)), 100) == 0
        assert size(ctypes.byref(_desc(n, 'heaqnn', (2, 1))), 100) == 0
    assert size(None, 100) == 0
    bad = _desc(7)
    bad.n_qubits = 0
    assert size(ctypes.byref(bad), 100) == 0
    for n in (7, 8, 9):
        # QuanONet (2, 1, 2, 1): 4 blocks of one sub-layer; HEAQNN (3, 0): three blocks without sub-layers
        for d, E, blk in ((_desc(n), 4 * n, 4), (_desc(n, 'heaqnn', (3, 0)), 3 * n, 0), (_desc(n, 'quanonet', (20, 2, 10, 2)), 30 * n, 60)):
            assert size(ctypes.byref(d), -1) == 0
            for B in (0, 1, 3, 100, 2048):
                got = size(ctypes.byref(d), B)
                assert got >= 2 * B * 4 ** n * 16
                assert got == _formula(lib, d, n, E, blk, B), (n, E, blk, B)
    # no 32-bit wrap: the matrices alone are 2^34 bytes at n = 9 and batch 2048
    assert size(ctypes.byref(_desc(9)), 2048) > 2 * 2048 * 4 ** 9 * 16 == 2 ** 34


def _loss_grad(lib, d, batch, nz, ham_diag=None, ws=None, ws_bytes=0, arrays=False):
    """the call with every array NULL (or, with `arrays`, a pointer nothing reads before the checks are through)"""
    p = ctypes.cast(ctypes.c_void_p(4096), ctypes.POINTER(ctypes.c_double)) if arrays else None
    return lib.qhea_model_loss_grad_noisy_exact_wide(None if d is None else ctypes.byref(d), batch, p, p, p, p, ham_diag,
                                                     None if nz is None else ctypes.byref(nz), 1.0, p, None, ws, ws_bytes, None)


def _train_steps(lib, d, n_steps, nz, first_step=1):
    return lib.qhea_model_train_steps_noisy_exact_wide(None if d is None else ctypes.byref(d), n_steps, None, None, None, None,
                                                       None, None, None if nz is None else ctypes.byref(nz), None, None, 0, None,
                                                       None, first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, 0, None)


def _full_train_steps(lib, d, nz, n_steps=2, first_step=1, row_begin=(0, 3, 5), ws=None, ws_bytes=0):
    """every array present (host memory: the checks read row_begin and nothing else); without a workspace nothing is launched"""
    from quanonet_amd import _lib
    P = _lib.model_param_count(d)
    buf = lambda k: (ctypes.c_double * k)()
    rb = (ctypes.c_int64 * 3)(*row_begin) if row_begin is not None else None
    return lib.qhea_model_train_steps_noisy_exact_wide(ctypes.byref(d), n_steps, rb, buf(64), buf(64), buf(8), buf(P), None,
                                                       ctypes.byref(nz), buf(2), buf(2 * (P + 2)), P + 2, buf(P), buf(P),
                                                       first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0, ws, ws_bytes, None)


def test_return_codes_without_gpu(lib):
    from quanonet_amd import _lib
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0)
    bads = (_lib.NoiseParams(-0.1, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.01, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
            _lib.NoiseParams(0, 0, float('nan'), 0, 1, 0), _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0))
    fake_ws = ctypes.c_void_p(1 << 20)                                   # never dereferenced: every call below returns first
    for n in (7, 8, 9):
        d = _desc(n)
        bad_desc = _desc(n)
        bad_desc.n_qubits = 0
        for call in (_loss_grad, _train_steps):
            assert call(lib, bad_desc, 10, ok) == -1
            assert call(lib, None, 10, ok) == -1
            assert call(lib, d, 0, ok) == 0                                       # empty batch / no steps
            assert call(lib, d, 0, _lib.NoiseParams(0.01, 0.02, 0.03, -5, 0, 9)) == 0     # shots, trajectories, seed are ignored
            for bad in bads:
                assert call(lib, d, 10, bad) == -1
            assert call(lib, d, 10, None) == -1                                   # no noise setting
            assert call(lib, d, -1, ok) == -1
            assert call(lib, d, 10, ok) == -1                                     # valid up to the NULL arrays
        assert _train_steps(lib, d, 3, ok, first_step=0) == -1
        # QHEA_EINVAL for a grid past 2^31 - 1 workgroups comes before QHEA_EWORKSPACE; one row fewer reaches the workspace check
        limit = INT_MAX >> (2 * (n - 6))
        assert _loss_grad(lib, d, limit + 1, ok, arrays=True) == -1
        assert _loss_grad(lib, d, limit + 1, ok, ws=fake_ws, ws_bytes=2 ** 63, arrays=True) == -1
        assert _loss_grad(lib, d, limit, ok, arrays=True) == -3
        # a short workspace: none, and one byte less than the size the library asks for
        need = lib.qhea_model_exact_noisy_wide_grad_workspace_bytes(ctypes.byref(d), 10)
        assert _loss_grad(lib, d, 10, ok, arrays=True) == -3
        assert _loss_grad(lib, d, 10, ok, ws=fake_ws, ws_bytes=need - 1, arrays=True) == -3
        assert _full_train_steps(lib, d, ok) == -3
        need = lib.qhea_model_exact_noisy_wide_grad_workspace_bytes(ctypes.byref(d), 3)    # the largest step has 3 rows
        assert _full_train_steps(lib, d, ok, ws=fake_ws, ws_bytes=need - 1) == -3
        assert _full_train_steps(lib, d, ok, row_begin=(0, limit + 1, limit + 2)) == -1
    for n in (2, 6, 10, 12):
        for d in (_desc(n), _desc(n, 'heaqnn', (2, 1))):
            for call in (_loss_grad, _train_steps):
                assert call(lib, d, 10, ok) == -2
                assert call(lib, d, 10, bads[0]) == -1                            # a bad rate is reported before the qubit count
    # X / Y read-outs do not combine with ham_diag (as in every other call)
    dx = _desc(7)
    dx.ham_pauli = 1
    assert _loss_grad(lib, dx, 10, ok, ham_diag=ctypes.cast(ctypes.c_void_p(256), ctypes.POINTER(ctypes.c_double))) == -1


def test_train_steps_two_faults_at_once(lib):
    """which code wins: first_step = 0 is refused with the descriptor, ahead of every other check (kStepCheckFirst, as the
    n <= 6 unit has it)"""
    from quanonet_amd import _lib
    d, d6, d10 = _desc(8), _desc(6), _desc(10)
    ok, bad, singular = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0), _lib.NoiseParams(0, 1.01, 0, 0, 1, 0), _lib.NoiseParams(0.75, 0, 0, 0, 1, 0)
    table = [('first_step 0, no row_begin', dict(d=d, nz=ok, first_step=0, row_begin=None), -1),
             ('first_step 0, invalid rate', dict(d=d, nz=bad, first_step=0), -1),
             ('first_step 0, n = 6', dict(d=d6, nz=ok, first_step=0), -1),
             ('first_step 0, refused amplification', dict(d=d, nz=singular, first_step=0), -1),
             ('first_step 0, no steps', dict(d=d, nz=ok, first_step=0, n_steps=0), -1),
             ('invalid rate, n = 10', dict(d=d10, nz=bad), -1),
             ('n = 6, refused amplification', dict(d=d6, nz=singular), -2),
             ('n = 6 alone', dict(d=d6, nz=ok), -2),
             ('n = 10 alone', dict(d=d10, nz=ok), -2),
             ('refused amplification, no workspace', dict(d=d, nz=singular), -2),
             ('descending row_begin, no workspace', dict(d=d, nz=ok, row_begin=(0, 4, 2)), -1),
             ('no workspace, a valid call of two steps', dict(d=d, nz=ok), -3)]
    for what, kw, want in table:
        assert _full_train_steps(lib, **kw) == want, what


def _closed_form(n, E, blk, p1, p2):
    return -((E + n * blk) * math.log10(1 - 4 * p1 / 3) + n * blk * math.log10(1 - 16 * p2 / 15))


def _rates_for(n, E, blk, target):
    """(p1, p2 = 6 p1) with log10 A = target"""
    lo, hi = 0.0, 0.9
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _closed_form(n, E, blk, mid / 6, mid) < target else (lo, mid)
    return lo / 6, lo


@pytest.mark.parametrize('n', [7, 8, 9])
def test_guard(lib, n):
    """7h's guard, unchanged: log10 A = 11.99 passes every check, 12.01 is refused before the empty batch is looked at"""
    from quanonet_amd import _lib
    d = _desc(n, 'quanonet', (20, 2, 10, 2))
    E, blk = 30 * n, 60
    amp = lambda nz: lib.qhea_model_exact_noisy_log10_amplification(ctypes.byref(d), ctypes.byref(nz))
    below, above = (_lib.NoiseParams(*_rates_for(n, E, blk, t), 0.01, 0, 1, 0) for t in (11.99, 12.01))
    assert abs(amp(below) - 11.99) < 1e-6 and abs(amp(above) - 12.01) < 1e-6
    assert _loss_grad(lib, d, 0, below) == 0 and _train_steps(lib, d, 0, below) == 0
    assert _loss_grad(lib, d, 10, below) == -1                                    # reaches the NULL arrays
    assert _loss_grad(lib, d, 10, below, arrays=True) == -3                       # ... and with them the workspace check
    assert _loss_grad(lib, d, 0, above) == -2 and _train_steps(lib, d, 0, above) == -2
    assert _loss_grad(lib, d, 10, above, arrays=True) == -2
    for nz in (_lib.NoiseParams(0.75, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 15 / 16, 0, 0, 1, 0)):       # singular channels
        assert amp(nz) == math.inf
        assert _loss_grad(lib, d, 0, nz) == -2 and _train_steps(lib, d, 0, nz) == -2


# ---- the tile maps under a trace -------------------------------------------------------------------------------------------------

def _tile_maps(n):
    """element -> (tile, local index) of stage A and stage B, as DESIGN.md 7t and hea_density_wide.hpp state them"""
    i = np.arange(1 << (2 * n), dtype=np.int64)
    a = (i >> 12, i & 4095)
    hi = 2 * n - 8                                                       # the first bit of wires n-4 .. n-1
    b = ((i >> 4) & ((1 << (hi - 4)) - 1), (i & 15) | ((i >> hi) << 4))
    return {'A': a, 'B': b}


def _hermitian(rng, D):
    m = rng.normal(size=(D, D)) + 1j * rng.normal(size=(D, D))
    return m + m.conj().T


@pytest.mark.parametrize('n', [7, 8])
def test_tile_shares_add_up_to_the_trace(n):
    """
    What a reverse stage does with a trace: a workgroup sums conj(O_i) (sigma_q rho)_i over the 4096 elements of its tile (both
    bits of wire q are local to it), the fold adds the tiles in tile order.  For Hermitian rho and O that is Im Tr(O sigma_q rho).
    """
    D, NE, tiles = 1 << n, 1 << (2 * n), 1 << (2 * (n - 6))
    rng = np.random.default_rng(n)
    rho, obs = _hermitian(rng, D) / D, _hermitian(rng, D)                # entries of order 1 / D, as a density matrix has
    i = np.arange(NE, dtype=np.int64)
    r = sum(((i >> (2 * w)) & 1) << w for w in range(n))                 # bit 2w: wire w's row bit, bit 2w + 1: its column bit
    c = sum(((i >> (2 * w + 1)) & 1) << w for w in range(n))
    flat_rho, flat_obs = rho[r, c], obs[r, c]
    shape = (1,) + (2,) * (2 * n)
    served = {'A': range(0, 6), 'B': range(6, n)}                        # the wires whose traces a stage takes
    for stage, q in (('A', 3), ('A', 0), ('B', n - 1), ('B', 6)):
        assert q in served[stage]
        tile, local = _tile_maps(n)[stage]
        assert np.unique(tile * 4096 + local).size == NE
        for ax in 'xyz':
            sig = DG.SIGMA[ax]
            want = np.imag(DG._trace(obs.reshape(shape), DG._left(rho.reshape(shape), n, q, sig), n))[0]
            # (sigma_q rho)_i = sum_j sigma[rb, j] rho_(i with wire q's row bit = j)
            rb = (i >> (2 * q)) & 1
            partner = [i & ~(1 << (2 * q)), i | (1 << (2 * q))]
            assert np.array_equal(tile[partner[0]], tile) and np.array_equal(tile[partner[1]], tile)     # local to the tile
            sr = sig[rb, 0] * flat_rho[partner[0]] + sig[rb, 1] * flat_rho[partner[1]]
            share = np.imag(np.conj(flat_obs) * sr)
            per_tile = np.array([share[tile == t].sum() for t in range(tiles)])
            total = 0.0
            for t in range(tiles):                                       # the fold: tile order 0, 1, ..
                total += per_tile[t]
            assert abs(total - want) <= 1e-13, (stage, q, ax, total, want)


# ---- the yardstick at the new size -----------------------------------------------------------------------------------------------

def _shift(n, cfgs, x, w, p, kw):
    """(value, d value / d x, d value / d w) per row by parameter shift through density_reference.final_rho"""
    val = lambda xx, ww: DR.exact_moments(n, cfgs, xx, ww, *p, **kw)[0]
    sx, sw = np.zeros(x.shape), np.zeros((x.shape[0],) + w.shape)
    for e in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, e] += np.pi / 2
        xm[:, e] -= np.pi / 2
        sx[:, e] = 0.5 * (val(xp, w) - val(xm, w))
    for idx in np.ndindex(w.shape):
        wp, wm = w.copy(), w.copy()
        wp[idx] += np.pi / 2
        wm[idx] -= np.pi / 2
        sw[(slice(None),) + idx] = 0.5 * (val(x, wp) - val(x, wm))
    return val(x, w), sx, sw


def test_helper_at_n7_against_parameter_shift():
    """circuit_grad at n = 7, stored and inverse walk, against parameter shift through density_reference.final_rho: the oracle
    of the GPU tests at the size they use it.  Blocks (7, 1), (7, 0): a first-sub-layer encoding and a block without sub-layers."""
    n, cfgs, p = 7, [(7, 1), (7, 0)], (0.03, 0.08, 0.04)
    rng = np.random.default_rng(7)
    x = rng.uniform(-np.pi, np.pi, (2, 14))
    w = rng.uniform(-np.pi, np.pi, (1, 3, n))
    kw = dict(offset=0.3, coeff=0.7, ham_pauli='Y')
    v, sx, sw = _shift(n, cfgs, x, w, p, kw)
    walks = {}
    for inverse in (False, True):
        v1, gx, gw = walks[inverse] = DG.circuit_grad(n, cfgs, x, w, *p, inverse=inverse, **kw)
        err = max(np.abs(v1 - v).max(), np.abs(gx - sx).max(), np.abs(gw - sw).max())
        print(f'n=7 inverse={inverse}: max|err against parameter shift|={err:.2e} max|g|={max(np.abs(sx).max(), np.abs(sw).max()):.2e}')
        assert err <= 1e-12
    diff = max(np.abs(a - b).max() for a, b in zip(walks[False], walks[True]))
    print(f'n=7 log10A={DG.log10_amplification(n, cfgs, p[0], p[1]):.2f}: inverse walk - stored walk = {diff:.2e}')
    assert diff <= 1e-12
