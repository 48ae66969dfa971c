"""
Every kernel QHEA_BWD_AUTO chooses, at the edges where the choice flips, against the C oracle on the whole batch.

``expected(n, cfgs, B, cus, ...)`` restates the automatic choice of hea_api.hip (kernel_inputs, then fwd_kernel_for and
bwd_kernel_for) in plain Python, in their order; each case captures the kernels its calls launch (tests/helpers.py: kernel_launches -- stream capture, the graph only
read) and asserts they are the ones ``expected`` names, then compares the results with the oracle.  If AUTO changes on
purpose, the table here changes with it.

  * circuit level, n = 2..5: sample groups at 1, 2 and 3 x the CU count, forward waves at 1 and 2 x the SIMD count, a half-full
    last group; block-unrolled and ragged shapes; the encoding widths either side of the ZYZ and split-layout limits; depths
    either side of the two-pipelines-per-workgroup LDS limit; n = 6..9 either side of the dense build; n = 10..12
  * read-outs X, Y and a diagonal Hamiltonian in every large-batch family
  * every forced variant by kernel name at the smallest shapes where the rules can differ
  * model level: model_train_steps (records the reduce kernel wrote) against oracle gradients + torch.optim.Adam, fused
    records on both sides of model_fuse_eligible; model_forward_chunks over 2.5 chunks of 16384 rows
"""
import copy
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from oracle import c_oracle as C
from tests.helpers import kernel_launches, mangled_is, oracle_adam_loop

pytestmark = pytest.mark.gpu

TOL = 1e-10                # out, grad_x, states
TOL_W = 1e-9               # grad_w for B <= 2100; beyond, 1e-12 x sum_b |g_b|
TOL_MODEL = 1e-9           # model-level rows and parameters

# ---------------------------------------------------------------------------------------------------------------------
# the automatic choice, restated (hea_api.hip, hea_zyz.hpp, hea_device.hpp, hea_inst.hip)
# ---------------------------------------------------------------------------------------------------------------------
Regime = namedtuple('Regime', 'fwd bwd pipes dense')

K_WAVES = 2                                  # hea_device.hpp kWaves (the forward / packed waves round up to it)
ZCS_BYTES = 20480                            # hea_zyz.hpp kZCsBytes
ZTRI2_FIXED = 2 * (4 * 3 * 1024) + 2 * 8 * 1024 + 1024 + 256 + 16 * 15 * 8   # ztri_fixed_lds(kZRingDepth<2> = 8): kBSlots = 4,
                                                                             # kRecBytes = 1024, kAxisRing = 16 (hea_zyz.hpp)
ZTRI2_LDS_LIMIT = 158 * 1024                 # hea_api.hip kernel_inputs: two_fit


def lane_bits(n):                            # hea_device.hpp lane_bits
    return n if n < 6 else 6


def padded_3n(n):                            # hea_device.hpp padded_3n
    return 8 if 3 * n <= 8 else 16 if 3 * n <= 16 else 32 if 3 * n <= 32 else 64


def zyz_eligible(n, E):                      # hea_zyz.hpp zyz_eligible: the (cos, sin) table of a sample group fits
    return 2 <= n <= 5 and (64 >> n) * (E + 2 * n) * 16 <= ZCS_BYTES


def fast_ld(n, cfgs):                        # hea_zyz.hpp zyz_fast_ld (Shape::fast_ld): every block enc = n, one ld in {1, 2}
    ld = cfgs[0][1]
    return ld if ld in (1, 2) and all(e == n and d == ld for e, d in cfgs) else 0


def zsplit_eligible(n, E, cfgs):             # hea_zyz.hpp zsplit_eligible
    return n == 5 and fast_ld(n, cfgs) != 0 and 2 * (E + 2 * n) * 32 <= ZCS_BYTES


def ztri2_lds(n, cfgs):                      # kernel_inputs, two_fit: LDS of bwd_ztri_kernel<N, 2>
    E, blk = O.circuit_sizes(n, cfgs)
    cs = (64 >> n) * (E + 2 * n) * (32 if zsplit_eligible(n, E, cfgs) else 16)
    return 2 * ZTRI2_FIXED + 2 * cs + blk * padded_3n(n) * 8


def expected(n, cfgs, B, cus, pauli='Z', state=False):
    """Regime(forward kernel, backward kernel, pipelines per workgroup, dense build) of a single-model call on B rows
    under QHEA_BWD_AUTO.  pauli: 'Z' (also a diagonal Hamiltonian), 'X' or 'Y'; state: the backward is given the final
    state.  In the order of hea_api.hip: what kernel_inputs leaves for the rules, then fwd_kernel_for, then bwd_kernel_for
    (single-model call: KernelInputs::single, CallTraits::R == 1)."""
    E, _ = O.circuit_sizes(n, cfgs)
    # kernel_inputs
    simd = 4 * cus                                                        # simd (simd_count)
    lds = n >= 10                                                         # lds (hea_lds.hip lds_supported)
    spw = 64 >> lane_bits(n)
    groups = -(-B // spw)                                                 # groups_d
    waves = -(-groups // K_WAVES) * K_WAVES                               # fwd_waves_d (also the packed backward's rows)
    records = zyz_eligible(n, E)                                          # records (AUTO runs the ZYZ kernels)
    fast = records and fast_ld(n, cfgs) != 0                              # fast
    srecords = records and zsplit_eligible(n, E, cfgs)                    # srecords
    two_fit = records and ztri2_lds(n, cfgs) <= ZTRI2_LDS_LIMIT           # two_fit
    # fwd_kernel_for
    shared = fast and waves > simd                                        # shared
    zyz = records and (shared or waves <= 2 * simd)                       # zyz
    if lds:
        fwd = 'lds_fwd_kernel'
    elif not zyz:
        fwd = 'fwd_kernel'
    elif shared:
        fwd = 'fwd_zshared_kernel'
    elif srecords and B <= simd and pauli == 'Z':                         # split forward; X / Y: the private-ring forward
        fwd = 'fwd_split_kernel'
    else:
        fwd = 'fwd_zyz_kernel'
    # bwd_kernel_for
    pipes, dense = 1, False
    pipelined = n <= 5 and 8 * groups <= 6 * simd                         # pipelined
    auto_two = cus < groups <= 2 * cus                                    # auto_two (= two_wanted, snap_wanted under AUTO)
    if lds:
        bwd = 'lds_bwd_kernel'
    elif fast and not pipelined:
        bwd = 'bwd_zpacked_kernel'
    elif not pipelined:
        bwd = 'bwd_kernel'
        dense = n in (8, 9) and waves > simd                              # dense_bit, hea_inst.hip launch_bwd_NN
    elif not records:
        bwd = 'bwd_tri_kernel'                                            # use_tri(): AUTO is the psi / lambda / sigma form
    elif auto_two and two_fit:
        pipes = 2                                                         # snapshot pipeline; X / Y / given state: ztri<N, 2>
        bwd = 'bwd_zsnap_kernel' if srecords and n == 5 and pauli == 'Z' and not state else 'bwd_ztri_kernel'
    elif srecords and groups <= cus and n == 5 and pauli == 'Z':          # quad_wanted; X / Y: ztri<N, 1>
        bwd = 'bwd_zquad_kernel'
    else:
        bwd = 'bwd_ztri_kernel'
    return Regime(fwd, bwd, pipes, dense)


def expected_fused(n, cfgs, B, cus):
    """whether model_train_steps' reduce kernel writes the next step's records (hea_api.hip model_fuse_blocks; steps of
    equal batch size)"""
    r = expected(n, cfgs, B, cus)
    if r.bwd not in ('bwd_ztri_kernel', 'bwd_zpacked_kernel', 'bwd_zsnap_kernel', 'bwd_zquad_kernel'):
        return False
    ld, kw = fast_ld(n, cfgs), padded_3n(n)
    _, blk = O.circuit_sizes(n, cfgs)
    if ld < 1:
        return False
    cols = ld * kw
    return cols in (16, 32) or (cols == 8 and (blk // ld) % 2 == 0)


FWD_KERNELS = ('fwd_split_kernel', 'fwd_zshared_kernel', 'fwd_zyz_kernel', 'fwd_kernel', 'lds_fwd_kernel')
BWD_KERNELS = ('bwd_zpacked_kernel', 'bwd_zsnap_kernel', 'bwd_zquad_kernel', 'bwd_ztri_kernel', 'bwd_tri_kernel',
               'bwd_pair_kernel', 'bwd_kernel', 'lds_bwd_kernel')


def _circuit_kernel(launches, idents):
    hits = [(ident, name, grid, block) for name, grid, block in launches for ident in idents if mangled_is(name, ident)]
    assert len(hits) == 1, [l[0] for l in launches]
    return hits[0]


def captured_regime(n, fwd_launches, bwd_launches):
    fwd = _circuit_kernel(fwd_launches, FWD_KERNELS)[0]
    bwd, name, _, _ = _circuit_kernel(bwd_launches, BWD_KERNELS)
    pipes = 2 if (mangled_is(name, 'bwd_ztri_kernel', (n, 2)) or bwd == 'bwd_zsnap_kernel') else 1
    dense = mangled_is(name, 'bwd_kernel', (n, 2))
    return Regime(fwd, bwd, pipes, dense)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
CUS_NOMINAL = 256          # (only to name the cases at collection time; every assertion takes the device's own count)


def _shapes(n):
    ragged = [(n, 1), (n - 1, 2), (n, 1), (n + 1, 1)]                      # not block-unrolled
    return {'unrolled2': [(n, 2)] * 3, 'unrolled1': [(n, 1)] * 4, 'ragged': ragged}


def _batch_edges(n):
    """(label, callable cus -> B) on each side of every edge: sample groups = 1, 2, 3 x CUs, forward waves = 1, 2 x SIMDs,
    and a half-full last group"""
    spw = 64 >> lane_bits(n)
    out = []
    for lab, k in (('groups=cus', 1), ('groups=2cus', 2), ('groups=3cus', 3), ('waves=simd', 4), ('waves=2simd', 8)):
        out.append((lab, lambda c, k=k: k * c * spw))
        out.append((lab + '+1', lambda c, k=k: k * c * spw + 1))
    out.append(('half-full-last', lambda c: 3 * c * spw - spw // 2))
    return out


CIRCUIT_CASES = []         # (id, n, cfgs, B(cus), read-outs)
for _n in (2, 3, 4, 5):
    for _sn, _cfgs in _shapes(_n).items():
        for _lab, _bf in _batch_edges(_n):
            CIRCUIT_CASES.append((f'n{_n}-{_sn}-{_lab}', _n, _cfgs, _bf, ('Z',)))
# encoding widths either side of the ZYZ limit (zyz_eligible: E <= 76 / 154 / 312 / 630) and the split limit (n = 5,
# zsplit_eligible: E <= 310), in blocks of enc = n
for _n, _nbs in ((2, (38, 39)), (3, (51, 52)), (4, (78, 79)), (5, (62, 63, 126, 127))):
    for _nb in _nbs:
        for _lab, _bf in (('pipelined', lambda c: 300), ('groups=3cus+1', lambda c, n=_n: 3 * c * (64 >> n) + 1)):
            CIRCUIT_CASES.append((f'n{_n}-E{_nb * _n}-{_lab}', _n, [(_n, 1)] * _nb, _bf, ('Z',)))
# n = 6..9: waves = SIMDs and one more (dense build for n = 8, 9), and B = 4096 with shallow circuits
for _n in (6, 7, 8, 9):
    _cfgs = [(_n, 2), (_n, 1)]
    CIRCUIT_CASES.append((f'n{_n}-waves=simd', _n, _cfgs, lambda c: 4 * c, ('Z',)))
    CIRCUIT_CASES.append((f'n{_n}-waves=simd+1', _n, _cfgs, lambda c: 4 * c + 1, ('Z',)))
    CIRCUIT_CASES.append((f'n{_n}-B4096', _n, [(_n, 1)] * 2, lambda c: 4096, ('Z',)))
# n = 10..12: B = 1024, ragged encodings
for _n, _cfgs in ((10, [(10, 1), (7, 2)]), (11, [(11, 1), (5, 1), (11, 1)]), (12, [(9, 1), (12, 1)])):
    CIRCUIT_CASES.append((f'n{_n}-B1024', _n, _cfgs, lambda c: 1024, ('Z',)))
# read-outs at large batch in every family: zpacked, the n = 5 two-pipeline range (Z: zsnap; X / Y / given state: ztri<5, 2>),
# the dense bwd_kernel and the workgroup-resident kernels
READOUTS = ('Z', 'X', 'Y', 'diag')
CIRCUIT_CASES += [
    ('readout-zpacked-n3', 3, [(3, 2)] * 3, lambda c: 3 * c * 8 + 100, READOUTS),
    ('readout-ztri2-n5', 5, [(5, 2)] * 3, lambda c: 3 * c, READOUTS),
    ('readout-ztri2-n4-ragged', 4, [(4, 1), (3, 1), (4, 2)], lambda c: 6 * c, READOUTS),
    ('readout-dense-n8', 8, [(8, 2), (8, 1)], lambda c: 4 * c + 76, READOUTS),
    ('readout-lds-n10', 10, [(10, 1), (7, 2)], lambda c: 1024, READOUTS),
]


def _depth_cases():
    """two depths either side of the two-pipeline LDS limit (kernel_inputs: two_fit), inside the two-pipeline batch range:
    two blocks of depth D (not block-unrolled for D > 2)"""
    out = []
    for n in (5, 3):
        D = 3
        while ztri2_lds(n, [(n, D + 1)] * 2) <= ZTRI2_LDS_LIMIT:
            D += 1
        for d in (D, D + 1):
            out.append((f'n{n}-depth{d}', n, [(n, d)] * 2, lambda c, n=n: 3 * c * (64 >> n) // 2, ('Z',)))
    return out


CIRCUIT_CASES += _depth_cases()


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _t(dev, a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


def _readout(n, ro, rng):
    """(ham_diag or None, pauli letter) of one read-out"""
    if ro == 'diag':
        return np.sort(rng.uniform(-3, 3, size=1 << n)), 'Z'
    return None, ro


def _capture_circuit(dev, n, cfgs, B, ro='Z', state=False):
    """the Regime the circuit calls of this case launch (inputs are immaterial to the choice)"""
    from quanonet_amd import _lib
    rng = np.random.default_rng(0)
    sh = _lib.CircuitShape(n, cfgs)
    E, blk = sh.E, sh.blk
    x, w, g = _t(dev, rng.uniform(-3, 3, (B, E))), _t(dev, rng.uniform(-3, 3, (blk, 3, n))), _t(dev, rng.normal(size=B))
    diag, pauli = _readout(n, ro, rng)
    dd = None if diag is None else _t(dev, diag)
    off, co = O.ham_params(n)
    st = _lib.hea_forward(sh, x, w, off, co, dd, return_state=True, ham_pauli=pauli)[1] if state else None
    fl = kernel_launches(dev, lambda: _lib.hea_forward(sh, x, w, off, co, dd, ham_pauli=pauli))
    bl = kernel_launches(dev, lambda: _lib.hea_backward(sh, x, w, g, off, co, dd, state=st, ham_pauli=pauli))
    return captured_regime(n, fl, bl)


@pytest.mark.parametrize('case', CIRCUIT_CASES, ids=[c[0] for c in CIRCUIT_CASES])
def test_circuit_regime_matches_oracle(dev, cus, case):
    from quanonet_amd import _lib
    name, n, cfgs, bf, readouts = case
    B = bf(cus)
    sh = _lib.CircuitShape(n, cfgs)
    E, blk = sh.E, sh.blk
    rng = np.random.default_rng(abs(hash(name)) % (1 << 31))
    x = rng.uniform(-np.pi, np.pi, (B, E)); w = rng.uniform(-np.pi, np.pi, (blk, 3, n)); g = rng.normal(size=B)
    xd, wd, gd = _t(dev, x), _t(dev, w), _t(dev, g)
    tol_w = TOL_W if B <= 2100 else 1e-12 * float(np.abs(g).sum())
    for ro in readouts:
        diag, pauli = _readout(n, ro, rng)
        dd = None if diag is None else _t(dev, diag)
        off, co = O.ham_params(n, -2.0, 3.0)
        out, st = _lib.hea_forward(sh, xd, wd, off, co, dd, return_state=True, ham_pauli=pauli)
        gx, gw, out2 = _lib.hea_backward(sh, xd, wd, gd, off, co, dd, want_out=True, ham_pauli=pauli)
        gx_s, gw_s = _lib.hea_backward(sh, xd, wd, gd, off, co, dd, state=st, ham_pauli=pauli)
        _lib.check_status(dev)
        ro_, rst = C.hea_forward(n, cfgs, x, w, off, co, diag, return_state=True, ham_pauli=pauli)
        _, rgx, rgw = C.hea_backward(n, cfgs, x, w, g, off, co, diag, ham_pauli=pauli)
        np.testing.assert_allclose(out.cpu().numpy(), ro_, rtol=0, atol=TOL, err_msg=f'{ro} out')
        np.testing.assert_allclose(st.cpu().numpy(), rst, rtol=0, atol=TOL, err_msg=f'{ro} state')
        np.testing.assert_allclose(out2.cpu().numpy(), ro_, rtol=0, atol=TOL, err_msg=f'{ro} backward out')
        for (a, b), what in (((gx, gw), ''), ((gx_s, gw_s), ' (given the state)')):
            np.testing.assert_allclose(a.cpu().numpy(), rgx, rtol=0, atol=TOL, err_msg=f'{ro} grad_x{what}')
            np.testing.assert_allclose(b.cpu().numpy(), rgw, rtol=0, atol=tol_w, err_msg=f'{ro} grad_w{what}')
        # the kernels: without and with the final state
        for state in (False, True):
            got = _capture_circuit(dev, n, cfgs, B, ro, state)
            assert got == expected(n, cfgs, B, cus, pauli, state), (ro, state, got)
        _lib.check_status(dev)


# ---------------------------------------------------------------------------------------------------------------------
# forced variants (qhea_set_backward_variant): the kernels by name at the smallest shapes where the rules can differ
# ---------------------------------------------------------------------------------------------------------------------
FORCED_VARIANTS = ('packed', 'pair', 'tri', 'ztri', 'zpacked', 'ztri2', 'zquad', 'zsnap')
_U5 = [(5, 2)] * 2         # block-unrolled and split-eligible; B = 3 is one and a half sample groups
FORCED_SHAPES = {          # id: (n, cfgs, B, read-out, backward given the final state)
    'q5': (5, _U5, 3, 'Z', False),
    'q5-X': (5, _U5, 3, 'X', False),                       # X read-out: zsnap / zquad / split forward fall back
    'q5-state': (5, _U5, 3, 'Z', True),                    # given final state: zsnap falls back
    'q3-ragged': (3, [(3, 1), (2, 2)], 9, 'Z', False),     # no fast ld: zpacked and zquad fall back
    'q6': (6, [(6, 1)], 2, 'Z', False),                    # no pipelined or ZYZ kernel exists
}
# Regime per variant and shape as the library of the commit BEFORE the kernel rules were gathered into fwd_kernel_for /
# bwd_kernel_for launched them on an MI355X (recorded, not derived from the code under test)
FORCED_EXPECTED = {
    'packed': {'q5': ('fwd_kernel', 'bwd_kernel', 1, False), 'q5-X': ('fwd_kernel', 'bwd_kernel', 1, False),
               'q5-state': ('fwd_kernel', 'bwd_kernel', 1, False), 'q3-ragged': ('fwd_kernel', 'bwd_kernel', 1, False),
               'q6': ('fwd_kernel', 'bwd_kernel', 1, False)},
    'pair': {'q5': ('fwd_kernel', 'bwd_pair_kernel', 1, False), 'q5-X': ('fwd_kernel', 'bwd_pair_kernel', 1, False),
             'q5-state': ('fwd_kernel', 'bwd_pair_kernel', 1, False), 'q3-ragged': ('fwd_kernel', 'bwd_pair_kernel', 1, False),
             'q6': ('fwd_kernel', 'bwd_kernel', 1, False)},
    'tri': {'q5': ('fwd_kernel', 'bwd_tri_kernel', 1, False), 'q5-X': ('fwd_kernel', 'bwd_tri_kernel', 1, False),
            'q5-state': ('fwd_kernel', 'bwd_tri_kernel', 1, False), 'q3-ragged': ('fwd_kernel', 'bwd_tri_kernel', 1, False),
            'q6': ('fwd_kernel', 'bwd_kernel', 1, False)},
    'ztri': {'q5': ('fwd_split_kernel', 'bwd_ztri_kernel', 1, False), 'q5-X': ('fwd_zyz_kernel', 'bwd_ztri_kernel', 1, False),
             'q5-state': ('fwd_split_kernel', 'bwd_ztri_kernel', 1, False), 'q3-ragged': ('fwd_zyz_kernel', 'bwd_ztri_kernel', 1, False),
             'q6': ('fwd_kernel', 'bwd_kernel', 1, False)},
    'zpacked': {'q5': ('fwd_zshared_kernel', 'bwd_zpacked_kernel', 1, False), 'q5-X': ('fwd_zshared_kernel', 'bwd_zpacked_kernel', 1, False),
                'q5-state': ('fwd_zshared_kernel', 'bwd_zpacked_kernel', 1, False), 'q3-ragged': ('fwd_zyz_kernel', 'bwd_kernel', 1, False),
                'q6': ('fwd_kernel', 'bwd_kernel', 1, False)},
    'ztri2': {'q5': ('fwd_split_kernel', 'bwd_ztri_kernel', 1, False), 'q5-X': ('fwd_zyz_kernel', 'bwd_ztri_kernel', 1, False),
              'q5-state': ('fwd_split_kernel', 'bwd_ztri_kernel', 1, False), 'q3-ragged': ('fwd_zyz_kernel', 'bwd_ztri_kernel', 1, False),
              'q6': ('fwd_kernel', 'bwd_kernel', 1, False)},
    'zquad': {'q5': ('fwd_split_kernel', 'bwd_zquad_kernel', 1, False), 'q5-X': ('fwd_zyz_kernel', 'bwd_ztri_kernel', 1, False),
              'q5-state': ('fwd_split_kernel', 'bwd_zquad_kernel', 1, False), 'q3-ragged': ('fwd_zyz_kernel', 'bwd_ztri_kernel', 1, False),
              'q6': ('fwd_kernel', 'bwd_kernel', 1, False)},
    'zsnap': {'q5': ('fwd_split_kernel', 'bwd_zsnap_kernel', 2, False), 'q5-X': ('fwd_zyz_kernel', 'bwd_ztri_kernel', 2, False),
              'q5-state': ('fwd_split_kernel', 'bwd_ztri_kernel', 2, False), 'q3-ragged': ('fwd_zyz_kernel', 'bwd_ztri_kernel', 2, False),
              'q6': ('fwd_kernel', 'bwd_kernel', 1, False)},
}
_FORCED_REF = {}


def _forced_reference(shape):
    """inputs and oracle results of one forced-variant shape, computed once"""
    if shape not in _FORCED_REF:
        n, cfgs, B, ro, _ = FORCED_SHAPES[shape]
        E, blk = O.circuit_sizes(n, cfgs)
        rng = np.random.default_rng(sorted(FORCED_SHAPES).index(shape))
        x = rng.uniform(-np.pi, np.pi, (B, E)); w = rng.uniform(-np.pi, np.pi, (blk, 3, n)); g = rng.normal(size=B)
        off, co = O.ham_params(n, -2.0, 3.0)
        ref_out, ref_st = C.hea_forward(n, cfgs, x, w, off, co, None, return_state=True, ham_pauli=ro)
        _, ref_gx, ref_gw = C.hea_backward(n, cfgs, x, w, g, off, co, None, ham_pauli=ro)
        _FORCED_REF[shape] = (x, w, g, off, co, ref_out, ref_st, ref_gx, ref_gw)
    return _FORCED_REF[shape]


@pytest.mark.parametrize('shape', list(FORCED_SHAPES))
@pytest.mark.parametrize('variant', FORCED_VARIANTS)
def test_forced_variant_kernels_and_oracle(dev, variant, shape):
    from quanonet_amd import _lib
    n, cfgs, B, ro, state = FORCED_SHAPES[shape]
    x, w, g, off, co, ref_out, ref_st, ref_gx, ref_gw = _forced_reference(shape)
    sh = _lib.CircuitShape(n, cfgs)
    xd, wd, gd = _t(dev, x), _t(dev, w), _t(dev, g)
    _lib.set_backward_variant(variant)
    try:
        out, st = _lib.hea_forward(sh, xd, wd, off, co, None, return_state=True, ham_pauli=ro)
        if state:
            (gx, gw), out2 = _lib.hea_backward(sh, xd, wd, gd, off, co, None, state=st, ham_pauli=ro), out
        else:
            gx, gw, out2 = _lib.hea_backward(sh, xd, wd, gd, off, co, None, want_out=True, ham_pauli=ro)
        _lib.check_status(dev)
        got = _capture_circuit(dev, n, cfgs, B, ro, state)
    finally:
        _lib.set_backward_variant('auto')
    assert got == Regime(*FORCED_EXPECTED[variant][shape]), got
    np.testing.assert_allclose(out.cpu().numpy(), ref_out, rtol=0, atol=TOL, err_msg='out')
    np.testing.assert_allclose(st.cpu().numpy(), ref_st, rtol=0, atol=TOL, err_msg='state')
    np.testing.assert_allclose(out2.cpu().numpy(), ref_out, rtol=0, atol=TOL, err_msg='backward out')
    np.testing.assert_allclose(gx.cpu().numpy(), ref_gx, rtol=0, atol=TOL, err_msg='grad_x')
    np.testing.assert_allclose(gw.cpu().numpy(), ref_gw, rtol=0, atol=TOL_W, err_msg='grad_w')


# ---------------------------------------------------------------------------------------------------------------------
# model level: model_train_steps against oracle gradients + torch.optim.Adam
# ---------------------------------------------------------------------------------------------------------------------
def _model(kind, n, net, b_in, t_in, seed, rng):
    from quanonet_amd.models import HEAQNNPT, QuanONetPT
    torch.manual_seed(seed)
    if kind == 'QuanONet':
        m = QuanONetPT(n, b_in, t_in, net, scale_coeff=0.1, if_trainable_freq=True)
        with torch.no_grad():
            m.branch_freq.bias.copy_(torch.from_numpy(rng.normal(scale=0.3, size=m.branch_freq.bias.shape)))
            m.trunk_freq.bias.copy_(torch.from_numpy(rng.normal(scale=0.3, size=m.trunk_freq.bias.shape)))
            m.bias.fill_(0.2)
        return m.double(), O.block_configs_quanonet(n, net)
    m = HEAQNNPT(n, b_in, net, scale_coeff=0.1, if_trainable_freq=True)
    with torch.no_grad():
        m.freq.bias.copy_(torch.from_numpy(rng.normal(scale=0.3, size=m.freq.bias.shape)))
    return m.double(), O.block_configs_heaqnn(n, net)


MODEL_CASES = [            # (id, kind, n, net, b_in, t_in, B(cus), steps)
    # one per regime family
    ('zquad-q5', 'QuanONet', 5, (2, 2, 1, 2), 8, 2, lambda c: c * 2, 3),
    ('zsnap-q5', 'QuanONet', 5, (2, 2, 1, 2), 8, 2, lambda c: 3 * c, 3),
    ('ztri1-q5', 'QuanONet', 5, (2, 2, 1, 2), 8, 2, lambda c: 5 * c, 3),
    ('ztri2-q4', 'QuanONet', 4, (2, 1, 1, 1), 8, 2, lambda c: 6 * c, 3),
    ('ztri2-q3-ragged', 'QuanONet', 3, (2, 2, 1, 1), 8, 2, lambda c: 12 * c, 3),
    ('zpacked-q2', 'QuanONet', 2, (2, 2, 2, 2), 8, 2, lambda c: 3 * c * 16 + 40, 2),
    ('tri-q2-wide', 'QuanONet', 2, (30, 1, 10, 1), 8, 2, lambda c: 2 * c * 16, 2),
    ('packed-q3-wide', 'QuanONet', 3, (40, 1, 20, 1), 8, 2, lambda c: 3 * c * 8 + 8, 2),
    ('dense-q9', 'HEAQNN', 9, (2, 1), 6, 0, lambda c: 4 * c + 1, 2),
    ('sparse-q9', 'HEAQNN', 9, (2, 1), 6, 0, lambda c: 4 * c, 2),
    ('q7-ragged', 'QuanONet', 7, (1, 2, 1, 1), 6, 2, lambda c: 4 * c + 100, 2),
    ('lds-q11', 'QuanONet', 11, (1, 1, 1, 2), 6, 2, lambda c: 1024, 2),
    # the reference grids under AUTO at B = 100
    ('grid-q2-net50-2-10-2', 'QuanONet', 2, (50, 2, 10, 2), 100, 1, lambda c: 100, 3),
    ('grid-q2-net200-2-300-2', 'QuanONet', 2, (200, 2, 300, 2), 100, 1, lambda c: 100, 3),
    ('grid-q3-net100-2-20-2', 'QuanONet', 3, (100, 2, 20, 2), 100, 1, lambda c: 100, 3),
    ('grid-q4-net100-2-50-2', 'QuanONet', 4, (100, 2, 50, 2), 100, 1, lambda c: 100, 3),
    ('grid-q5-net100-2-50-2', 'QuanONet', 5, (100, 2, 50, 2), 100, 1, lambda c: 100, 3),
    # cfg 2's model at B = 4096 (zpacked, fused records); cfg 4's HEAQNN Q8 (20, 2) at B = 2048 (dense)
    ('cfg2-B4096', 'QuanONet', 5, (40, 2, 20, 2), 100, 2, lambda c: 4096, 2),
    ('cfg4-B2048', 'HEAQNN', 8, (20, 2), 20, 0, lambda c: 2048, 2),
    # either side of model_fuse_eligible: n = 2 with one sub-layer per block fuses with an even block count only
    ('fuse-q2-net5-1-5-1', 'QuanONet', 2, (5, 1, 5, 1), 8, 1, lambda c: 3000, 3),
    ('nofuse-q2-net5-1-4-1', 'QuanONet', 2, (5, 1, 4, 1), 8, 1, lambda c: 3000, 3),
]


def _model_data(kind, b_in, t_in, rows, rng):
    branch = rng.normal(size=(rows, b_in))
    trunk = rng.uniform(size=(rows, t_in)) if kind == 'QuanONet' else None
    return branch, trunk, rng.normal(scale=0.5, size=rows)


def _train_call(dev, model, kind, branch, trunk, y, bounds, gbs, lr):
    """(call, (params, rows)) of model_train_steps on fresh device copies"""
    from quanonet_amd import _lib
    desc = model.fused_desc()
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).to(dev).contiguous()
    P = params.numel()
    m_, v_ = torch.zeros_like(params), torch.zeros_like(params)
    rows = torch.zeros(len(gbs), P + 2, dtype=torch.float64, device=dev)
    bd, td = _t(dev, branch), (_t(dev, trunk) if trunk is not None else None)
    yd = _t(dev, y)

    def call():
        _lib.model_train_steps(desc, bounds, gbs, bd, td, yd, params, rows, m_, v_, 1, lr, 0.9, 0.999, 1e-8, 0.0)
    return call, (params, rows)


@pytest.mark.parametrize('case', MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_model_train_steps_regime_matches_oracle_and_adam(dev, cus, case):
    from quanonet_amd import _lib
    name, kind, n, net, b_in, t_in, bf, steps = case
    B = bf(cus)
    rng = np.random.default_rng(abs(hash(name)) % (1 << 31))
    model, cfgs = _model(kind, n, net, b_in, t_in, 5, rng)
    branch, trunk, y = _model_data(kind, b_in, t_in, steps * B, rng)
    bounds, gbs, lr = [i * B for i in range(steps + 1)], [B] * steps, 2e-3
    cpu_model = copy.deepcopy(model)
    names = [k for k, _ in cpu_model.named_parameters()]
    want_rows, want_p = oracle_adam_loop(cpu_model, names, branch, trunk, y, bounds, gbs, n, net, lr, model_type=kind)

    call, (params, rows) = _train_call(dev, model, kind, branch, trunk, y, bounds, gbs, lr)
    call()
    _lib.check_status(dev)
    got = rows.cpu().numpy()
    for i in range(steps):
        np.testing.assert_allclose(got[i], want_rows[i], rtol=0, atol=TOL_MODEL, err_msg=f'step {i}')
    np.testing.assert_allclose(params.cpu().numpy(), want_p, rtol=0, atol=TOL_MODEL)
    assert np.abs(want_rows[0][:-2] - want_rows[-1][:-2]).max() > 1e-7          # the steps did move the parameters

    # the kernels: the backward kernel of the circuit regime in every step, and the prep launch dropped after a step whose
    # reduce kernel wrote the records (fused)
    call, _ = _train_call(dev, model, kind, branch, trunk, y, bounds, gbs, lr)
    launches = kernel_launches(dev, call)
    want = expected(n, cfgs, B, cus)
    bwd = [l for l in launches if any(mangled_is(l[0], k) for k in BWD_KERNELS)]
    assert len(bwd) == steps and all(mangled_is(l[0], want.bwd) for l in bwd), ([l[0] for l in bwd], want)
    for l in bwd:
        assert mangled_is(l[0], 'bwd_ztri_kernel', (n, 2)) == (want.bwd == 'bwd_ztri_kernel' and want.pipes == 2)
        assert mangled_is(l[0], 'bwd_kernel', (n, 2)) == want.dense
    preps = [l for l in launches if mangled_is(l[0], 'prep_zyz_kernel') or mangled_is(l[0], 'prep_model_kernel')]
    fused = [l for l in launches if '19reduce_model_kernelILb1E' in l[0]]          # reduce_model_kernel<FUSE = true, ...>
    if expected_fused(n, cfgs, B, cus):
        assert len(preps) == 1 and len(fused) == steps - 1, ([l[0] for l in launches])
    else:
        assert len(preps) == steps and not fused, ([l[0] for l in launches])
    _lib.check_status(dev)


# ---------------------------------------------------------------------------------------------------------------------
# evaluation path: model_forward_chunks, 2.5 chunks of 16384 rows
# ---------------------------------------------------------------------------------------------------------------------
CHUNK = 16384
EVAL_CASES = [
    ('q2-net5-1-5-1', 2, (5, 1, 5, 1), 100, 1),              # the shipped checkpoint's shape
    ('q5-net40-2-20-2', 5, (40, 2, 20, 2), 100, 2),          # cfg 2
    ('q5-net10-2-5-1', 5, (10, 2, 5, 1), 20, 2),             # not block-unrolled: the first-generation forward at 16384 rows
]


@pytest.mark.parametrize('case', EVAL_CASES, ids=[c[0] for c in EVAL_CASES])
def test_forward_chunks_match_oracle_on_every_row(dev, cus, case):
    from quanonet_amd import _lib
    name, n, net, b_in, t_in = case
    rng = np.random.default_rng(abs(hash(name)) % (1 << 31))
    model, cfgs = _model('QuanONet', n, net, b_in, t_in, 9, rng)
    N = 2 * CHUNK + CHUNK // 2 + 3
    branch, trunk, _ = _model_data('QuanONet', b_in, t_in, N, rng)
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    want = O.quanonet_forward(sd, branch, trunk, n, net, engine=C)
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).to(dev).contiguous()
    bd, td = _t(dev, branch), _t(dev, trunk)
    desc = model.fused_desc()
    got = _lib.model_forward_chunks(desc, bd, td, params, CHUNK)
    _lib.check_status(dev)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=TOL)
    # the forward kernel of each chunk is the circuit regime's at that chunk's rows
    launches = kernel_launches(dev, lambda: _lib.model_forward_chunks(desc, bd, td, params, CHUNK))
    fwd = [_circuit_kernel([l], FWD_KERNELS)[0] for l in launches if any(mangled_is(l[0], k) for k in FWD_KERNELS)]
    sizes = [CHUNK, CHUNK, N - 2 * CHUNK]
    assert fwd == [expected(n, cfgs, s, cus).fwd for s in sizes], fwd
    _lib.check_status(dev)


# ---------------------------------------------------------------------------------------------------------------------
# coverage: the cases above reach every regime expected() can return for n <= 9
# ---------------------------------------------------------------------------------------------------------------------
def _all_regimes(cus):
    """every (fwd, bwd, pipes, dense) expected() returns for n <= 9 over a sweep of shapes, batches and read-outs"""
    out = set()
    for n in range(2, 10):
        shapes = list(_shapes(n).values()) if n <= 5 else [[(n, 1)] * 2]
        if n <= 5:
            shapes += [[(n, 1)] * nb for nb in {2: (38, 39), 3: (51, 52), 4: (78, 79), 5: (62, 63, 126, 127)}[n]]
            shapes += [[(n, 300)] * 2]
        spw = 64 >> lane_bits(n)
        batches = sorted({max(1, int(k * cus * spw)) + d for k in (0.25, 0.5, 1, 1.5, 2, 2.5, 3, 4, 6, 8, 9) for d in (0, 1)})
        for cfgs in shapes:
            for B in batches:
                for pauli in ('Z', 'X'):
                    for state in (False, True):
                        out.add(expected(n, cfgs, B, cus, pauli, state))
    return out


def test_cases_cover_every_regime(dev, cus):
    from quanonet_amd import _lib
    seen = set()
    for name, n, cfgs, bf, readouts in CIRCUIT_CASES:
        if n > 9:
            continue
        B = bf(cus)
        for ro in readouts:
            pauli = 'Z' if ro == 'diag' else ro
            for state in (False, True):
                r = expected(n, cfgs, B, cus, pauli, state)
                if r not in seen:
                    got = _capture_circuit(dev, n, cfgs, B, ro, state)
                    assert got == r, (name, ro, state, got)
                    seen.add(got)
    _lib.check_status(dev)
    missing = _all_regimes(cus) - seen
    assert not missing, sorted(missing)


def test_expected_table_fixed_points():
    """the restated rules at 256 CUs (MI355X): fixed points of the regime table in DESIGN.md section 3.0"""
    c = CUS_NOMINAL
    u5, u3 = [(5, 2)] * 3, [(3, 1)] * 4
    assert expected(5, u5, 512, c) == Regime('fwd_split_kernel', 'bwd_zquad_kernel', 1, False)
    assert expected(5, u5, 513, c) == Regime('fwd_split_kernel', 'bwd_zsnap_kernel', 2, False)
    assert expected(5, u5, 800, c, 'X') == Regime('fwd_zyz_kernel', 'bwd_ztri_kernel', 2, False)
    assert expected(5, u5, 1025, c) == Regime('fwd_zyz_kernel', 'bwd_ztri_kernel', 1, False)
    assert expected(5, u5, 1537, c).bwd == 'bwd_zpacked_kernel'
    assert expected(5, u5, 2049, c).fwd == 'fwd_zshared_kernel'
    assert expected(3, u3, 3000, c).pipes == 2 and expected(3, u3, 4097, c).pipes == 1
    assert expected(5, [(5, 1)] * 127, 100, c).bwd == 'bwd_tri_kernel'
    assert expected(5, [(5, 1)] * 126, 100, c).bwd == 'bwd_ztri_kernel'
    assert expected(8, [(8, 1)], 1024, c).dense is False and expected(8, [(8, 1)], 1025, c).dense is True
    assert expected(6, [(6, 1)], 1025, c) == Regime('fwd_kernel', 'bwd_kernel', 1, False)
    assert expected(5, [(5, 1), (4, 1)], 2 * 2 * 4 * c + 2, c).fwd == 'fwd_kernel'
    assert expected_fused(2, [(2, 1)] * 10, 3000, c) and not expected_fused(2, [(2, 1)] * 9, 3000, c)
