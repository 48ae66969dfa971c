"""
Member launches (qhea_model_{ensemble,sweep,depth_sweep,qubit_sweep}_train_steps) at the edges of their automatic kernel choice
and past the 64-member fill chunks, every member against the C oracle + torch.optim.Adam.

``expected_member(entry, descs, R, schedule, cus)`` restates how the four entry points choose their path and kernels (hea_api.hip:
members_train_steps, depth_grid_steps, qhea_model_qubit_sweep_train_steps); each case captures the kernels its call launches
(tests/helpers.py: kernel_launches -- stream capture, the graph only read) and asserts they are the ones ``expected_member``
names, then checks every member over two steps, the second one short: its [grads | sse | sum y^2] rows, parameters and Adam
moments against the oracle and torch.optim.Adam, and the NaN sentinel in the row tails beyond its vector.

  * ensembles and sweeps, n = 2..5: R x sample groups at 1, 2 and 3 x the CU count and one step beyond, reached by R at a fixed
    batch and by the batch at a fixed R; odd group counts under two pipelines; last zpacked workgroups of 1 and kZPWaves - 1
    groups; depths either side of the two-pipeline LDS limit; encoding widths either side of the ZYZ limit; a ragged shape past
    3 x CUs; schedules whose steps differ in path or kernel; both sides of fused records; a Y member at the zquad edge; R = 1 at
    the snapshot pipeline
  * n = 7 (R calls in sequence, status folded into slice 0's header) and n = 10 (the workgroup-resident member grid)
  * depth and qubit sweeps at n = 8, 9 with R x waves at the SIMD count and beyond it (dense bwd_kernel off / on)
  * R = 64, 65, 130 for each entry point, every member with its own read-out, learning rate, scale and (where allowed) depth,
    bitwise its single-model run; the README's capacity (80), scaling (330) and circuit (120) grids at their full size
  * a 66-member SweepSolver against the PTSolver runs of members 0, 63, 64 and the last one
If the automatic choice changes on purpose, the rules here change with it (member launches).
"""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from tests.helpers import (flat, heaqnn, kernel_launches, mangled_is, member_call, member_data, member_lossgrad, oracle_adam_state,
                           quanonet, run_members, run_single)
from tests.test_dispatch_regimes import (CUS_NOMINAL, ZTRI2_LDS_LIMIT, expected, expected_fused, lane_bits, padded_3n,
                                         ztri2_lds)

TOL = 1e-10
ADAM_EPS = 1e-8                      # (helpers.member_call, torch.optim.Adam's default)
K_WAVES = 2                          # hea_device.hpp:33 kWaves
K_MEMBER_FILL = 64                   # hea_api.hip:1340 kMemberFill
K_WORK_FILL = 256                    # hea_api.hip:1364 kWorkFill
K_FREQ_COLS = 8                      # hea_api.hip:828 kFreqCols
ZYZ_BWD = ('bwd_zpacked_kernel', 'bwd_zsnap_kernel', 'bwd_zquad_kernel', 'bwd_ztri_kernel')
QUANONET, HEAQNN = 0, 1              # _lib.MODEL_QUANONET / MODEL_HEAQNN

# ---------------------------------------------------------------------------------------------------------------------
# the automatic choice of the member entry points, restated
# ---------------------------------------------------------------------------------------------------------------------
# path:  'grid' (one launch per kernel, member = blockIdx.y), 'depth_grid' (depth_grid_steps: depth sweeps, and ensembles /
#        sweeps at n >= 10), 'qubit_grid' (qubit sweeps), 'sequential' (R qhea_model_train_steps calls)
# bwd:   the call's backward launches in launch order, (kernel, template arguments or None, form, gridDim.y); form is the
#        argument type of the member instantiation ('ZBwdArgsM', 'DepthArgs', 'QubitArgs') or 'single' / 'class'
# preps: prep launches; fused: reduce launches that write the next step's records; member_fills / work_fills /
#        folds: member_fill_kernel, work_fill_kernel and status_fold_kernel launches
MemberRegime = namedtuple('MemberRegime', 'path bwd preps fused member_fills work_fills folds')
FORMS = ('ZBwdArgsM', 'DepthArgs', 'QubitArgs')


def _cfgs(d):
    """the member's circuit blocks (hea_oracle: trunk blocks first)"""
    net = list(d.net)
    return O.block_configs_quanonet(d.n_qubits, net) if d.model == QUANONET else O.block_configs_heaqnn(d.n_qubits, net[:2])


def _pauli(d):
    return 'ZXY'[d.ham_pauli]


def _single_launch(n, cfgs, nb, cus, pauli, form='single', gy=1, zsnap_ok=True):
    """(kernel, targs, form, gridDim.y) of one model-level backward launch at the regime of Bd = nb rows (expected())"""
    r = expected(n, cfgs, nb, cus, pauli)
    if r.bwd == 'bwd_zsnap_kernel' and not zsnap_ok:           # :650 B == Bd, :741 R == 1: member launches take ztri<5, 2>
        return ('bwd_ztri_kernel', (n, 2), form, gy)
    targs = {'bwd_ztri_kernel': (n, r.pipes), 'bwd_zpacked_kernel': (n,), 'bwd_kernel': (n, 2 if r.dense else 1),
             'bwd_tri_kernel': (n,), 'lds_bwd_kernel': (n,)}.get(r.bwd)
    return (r.bwd, targs, form, gy)


def _nwaves(n, nb):                                           # hea_qsweep.hpp:27 qs_nwaves, hea_api.hip:2111
    spw = 64 >> lane_bits(n)
    return -(-(-(-nb // spw)) // K_WAVES) * K_WAVES


def _counts(d):                                               # hea_api.hip:2099 depth_counts: (c0, ld0), (c1, ld1)
    net = list(d.net)
    if d.model == QUANONET:
        return (net[2], net[3]), (net[0], net[1])
    return (net[0], net[1]), (0, 0)


def _red_roles(d):                                            # hea_api.hip:2344 red_roles (:303 red_cols)
    n, kw = d.n_qubits, padded_3n(d.n_qubits)
    (c0, l0), (c1, l1) = _counts(d)
    blk, E = c0 * l0 + c1 * l1, n * (c0 + c1)
    return -(-blk * kw // max(16, kw)) + (-(-E // K_FREQ_COLS) if d.trainable_freq else 0) + 1


def expected_member(entry, descs, R, sched, cus):
    """MemberRegime of one call under QHEA_BWD_AUTO.  entry: 'ensemble', 'sweep', 'depth' or 'qubit'; descs: the R members'
    descriptors (an ensemble's all equal; a sweep's differ in read-out and scale only); sched: the steps' row counts."""
    simd = 4 * cus                                            # :519 simd_count
    steps = len(sched)
    fills = -(-R // K_MEMBER_FILL)                            # :1961, :2139, :2455 one launch per kMemberFill members
    d0 = descs[0]
    n = d0.n_qubits
    if entry == 'depth':                                      # :2277 always depth_grid_steps
        return _depth_grid(descs, R, sched, simd, fills)
    if entry == 'qubit':
        return _qubit_grid(descs, R, sched, simd, fills)
    cfgs = _cfgs(d0)
    # :1955-1960 one X / Y member gives the launch the kernels of an X model (R > 1); R = 1 runs member 0's descriptor
    lp = 'Z' if all(_pauli(d) == 'Z' for d in descs) else 'X'
    lp = _pauli(d0) if R == 1 else lp
    # :1916-1921 one grid iff every step's layout for R x nb rows takes the ZYZ kernels (:1333 ensemble_grid)
    grid = R <= 65535 and all(expected(n, cfgs, R * nb, cus, lp).bwd in ZYZ_BWD for nb in sched)
    if not grid and R > 1 and n >= 10:                        # :1927 (n = 10..12 members: members_lds_grid)
        return _depth_grid(descs, R, sched, simd, fills)
    if not grid:                                              # :1933-1951 R model_train_steps calls, status folded
        bwd, preps, fused = [], 0, 0
        for d in descs:
            ready = False
            for i, nb in enumerate(sched):                    # :1821-1835 qhea_model_train_steps
                nxt = i + 1 < steps and sched[i + 1] == nb and expected_fused(n, cfgs, nb, cus)
                bwd.append(_single_launch(n, cfgs, nb, cus, _pauli(d)))
                preps += 0 if ready else 1
                fused += 1 if nxt else 0
                ready = nxt
        return MemberRegime('sequential', tuple(bwd), preps, fused, 0, 0, R - 1)
    bwd, preps, fused, ready = [], 0, 0, False
    for i, nb in enumerate(sched):                            # :1972-1987
        nxt = i + 1 < steps and sched[i + 1] == nb and expected_fused(n, cfgs, R * nb, cus)   # :1976 on the R x nb layout
        if R > 1:                                             # :730 gridDim.y = R: the member instantiations (hea_inst.hip)
            bwd.append(_single_launch(n, cfgs, R * nb, cus, lp, 'ZBwdArgsM', R, zsnap_ok=False))
        else:
            bwd.append(_single_launch(n, cfgs, nb, cus, lp))
        preps += 0 if ready else 1
        fused += 1 if nxt else 0
        ready = nxt
    return MemberRegime('grid', tuple(bwd), preps, fused, fills if R > 1 else 0, 0, 0)


def _depth_grid(descs, R, sched, simd, fills):
    """depth_grid_steps (:2128): member fills, then per step one prep, one backward and one reduce launch"""
    n = descs[0].n_qubits
    bwd = []
    for nb in sched:
        if n >= 10:                                           # :2185 one workgroup per (sample, member)
            bwd.append(('lds_bwd_kernel', (n,), 'DepthArgs', R))
        else:                                                 # :2181 dense iff R x nwaves > SIMDs (built for n = 8, 9)
            dense = n in (8, 9) and R * _nwaves(n, nb) > simd
            bwd.append(('bwd_kernel', (n, 2 if dense else 1), 'DepthArgs', R))
    return MemberRegime('depth_grid', tuple(bwd), len(sched), 0, fills, 0, 0)


def _qubit_grid(descs, R, sched, simd, fills):
    """qhea_model_qubit_sweep_train_steps (:2418): member fills, work fills (qubit_plan :2348), then per step one prep, one launch
    per register class present, one per n = 7..9 and per n = 10..12 present, one reduce"""
    bmax = max(sched)
    ns = [d.n_qubits for d in descs]
    entries = sum(_nwaves(m, bmax) // K_WAVES for m in ns if m <= 6)        # :2350-2361 (member, sample group)
    entries += sum(1 for m in ns if m >= 7)                                 # :2362-2376 (member, 0)
    entries += sum(_red_roles(d) for d in descs)                            # :2377-2379 (member, role)
    bwd = []
    for nb in sched:
        for lo, hi in ((2, 2), (3, 6)):                                     # :2506-2512, hea_qsweep.hpp:18-20
            if any(lo <= m <= hi for m in ns):
                bwd.append(('bwd_qsweep_kernel', (lo, hi, 1), 'class', 1))
        for m in (7, 8, 9):                                                 # :2513-2532, dense iff cnt x nw > SIMDs (:2523)
            cnt = ns.count(m)
            if cnt:
                dense = m in (8, 9) and cnt * _nwaves(m, nb) > simd
                bwd.append(('bwd_kernel', (m, 2 if dense else 1), 'QubitArgs', cnt))
        for m in (10, 11, 12):                                              # :2533-2546
            cnt = ns.count(m)
            if cnt:
                bwd.append(('lds_bwd_kernel', (m,), 'QubitArgs', cnt))
    return MemberRegime('qubit_grid', tuple(bwd), len(sched), 0, fills, -(-entries // K_WORK_FILL), 0)


BWD_IDENTS = ('bwd_zpacked_kernel', 'bwd_zsnap_kernel', 'bwd_zquad_kernel', 'bwd_ztri_kernel', 'bwd_tri_kernel',
              'bwd_pair_kernel', 'bwd_kernel', 'lds_bwd_kernel', 'bwd_qsweep_kernel')


def captured_member(launches, want):
    """the MemberRegime a captured call shows, given the expected one (whose path and template arguments name what to read)"""
    bwd = []
    for name, grid, _ in launches:
        hit = [k for k in BWD_IDENTS if mangled_is(name, k)]
        if not hit:
            continue
        assert len(hit) == 1, name
        k = hit[0]
        form = next((f for f in FORMS if f'{len(f)}{f}' in name), 'class' if k == 'bwd_qsweep_kernel' else 'single')
        bwd.append((k, name, form, grid[1]))
    # template arguments: the expected ones if the name carries them, else the name itself (the assertion then shows it)
    got = []
    for i, (k, name, form, gy) in enumerate(bwd):
        w = want.bwd[i] if i < len(want.bwd) else None
        targs = w[1] if (w is not None and w[0] == k and (w[1] is None or mangled_is(name, k, w[1]))) else name
        got.append((k, targs, form, gy))
    count = lambda ident: sum(1 for l in launches if mangled_is(l[0], ident))
    preps = sum(count(k) for k in ('prep_zyz_kernel', 'prep_model_kernel', 'prep_model_depth_kernel', 'prep_model_qubit_kernel'))
    fused = sum(1 for l in launches if '19reduce_model_kernelILb1E' in l[0])      # reduce_model_kernel<FUSE = true, ...>
    return MemberRegime(want.path, tuple(got), preps, fused, count('member_fill_kernel'), count('work_fill_kernel'),
                        count('status_fold_kernel'))


# ---------------------------------------------------------------------------------------------------------------------
# members: a cell is one member's model and hyper-parameters
# ---------------------------------------------------------------------------------------------------------------------
Cell = namedtuple('Cell', 'kind n net seed pauli hb scale trainable lr diag')


def cell(n, net, seed=0, kind='QuanONet', pauli='Z', hb=(-5.0, 5.0), scale=0.1, trainable=True, lr=1e-3, diag=None):
    return Cell(kind, n, tuple(net), seed, pauli, tuple(hb), scale, trainable, lr, diag)


def _model(c, b_in, t_in):
    kw = dict(scale_coeff=c.scale, if_trainable_freq=c.trainable, ham_bound=c.hb, ham_pauli=c.pauli)
    if c.diag is not None:
        kw['ham_diag'] = np.asarray(c.diag, np.float64)
    if c.kind == 'QuanONet':
        return quanonet(c.n, b_in, t_in, c.net, c.seed, **kw)
    return heaqnn(c.n, b_in, c.net, c.seed, **kw)


def _lossgrad(c):
    return member_lossgrad(c.kind, c.n, c.net, ham_bound=c.hb, ham_pauli=c.pauli, ham_diag=c.diag,
                           scale_coeff=None if c.trainable else c.scale)


def _widths(cells, b_in, t_in):
    return (b_in, t_in) if cells[0].kind == 'QuanONet' else (b_in,)


def _diags(entry, cells):
    if all(c.diag is None for c in cells):
        return None
    return cells[0].diag if entry == 'ensemble' else [c.diag for c in cells]


class Members:
    """R members of one call: models, data and the schedule"""

    def __init__(self, entry, cells, sched, seed, b_in=6, t_in=2):
        self.entry, self.cells, self.sched = entry, cells, list(sched)
        self.bounds = [0]
        for s in self.sched:
            self.bounds.append(self.bounds[-1] + s)
        self.models = [_model(c, b_in, t_in) for c in cells]
        self.inputs, self.ys = member_data(len(cells), self.bounds[-1], _widths(cells, b_in, t_in), seed)
        self.lrs = [c.lr for c in cells]
        self.hd = _diags(entry, cells)

    def call(self, dev, **kw):
        return member_call(dev, self.entry, self.models, self.lrs, self.inputs, self.ys, self.bounds, self.sched,
                           ham_diag=self.hd, **kw)

    def run(self, dev):
        """(params, exp_avg, exp_avg_sq, rows) with NaN beyond each member's vector and three NaN columns past the rows"""
        return run_members(dev, self.entry, self.models, self.lrs, self.inputs, self.ys, self.bounds, self.sched,
                           ham_diag=self.hd, sentinel=float('nan'), rows_sentinel=float('nan'), rows_extra=3)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max()))) if a.size else 0.0


def check_kernels(dev, cus, ms):
    want = expected_member(ms.entry, [m.fused_desc() for m in ms.models], len(ms.models), ms.sched, cus)
    call, _ = ms.call(dev)
    got = captured_member(kernel_launches(dev, call), want)
    assert got == want, (got, want)
    return want


def check_oracle(got, ms, members=None):
    """every member (or those listed) against the oracle + torch.optim.Adam; NaN tails untouched.  Returns the worst error."""
    params, m1, m2, rows = (t.numpy() for t in got)
    worst = 0.0
    for i in (range(len(ms.models)) if members is None else members):
        c, model = ms.cells[i], ms.models[i]
        want_rows, want_p, want_m1, want_m2 = oracle_adam_state(model, _lossgrad(c), ms.inputs[i], ms.ys[i], ms.bounds,
                                                                ms.sched, c.lr)
        P = want_p.size
        errs = (_rel(rows[i][:, :P + 2], want_rows), _rel(m1[i][:P], want_m1), _rel(m2[i][:P], want_m2))
        assert max(errs) < TOL, (i, c, errs)
        # the parameters: Adam's first step moves a parameter by lr g / (|g| + eps), whose slope lr / eps (3e5 at lr = 3e-3)
        # turns a rounding-level gradient difference near g = 0 into a visible one; beyond TOL, only that much is allowed
        err_g = float(np.abs(rows[i][:, :P] - want_rows[:, :P]).max())
        err_p = float(np.abs(params[i][:P] - want_p).max())
        assert err_p < TOL + len(ms.sched) * c.lr / ADAM_EPS * err_g, (i, c, err_p, err_g)
        worst = max(worst, *errs)
        assert np.isnan(rows[i][:, P + 2:]).all(), (i, 'gradient row tail written')
        for t, what in ((params, 'params'), (m1, 'exp_avg'), (m2, 'exp_avg_sq')):
            assert np.isnan(t[i][P:]).all(), (i, what, 'row tail written')
    assert np.abs(want_rows[0][:-2] - want_rows[-1][:-2]).max() > 1e-8          # the steps moved the parameters
    return worst


def check_bitwise(dev, got, ms, variant):
    """every member bitwise its own model_train_steps run under `variant` (got: the call's results under that variant)"""
    from quanonet_amd import _lib
    params, m1, m2, rows = got
    _lib.set_backward_variant(variant)
    try:
        for i, model in enumerate(ms.models):
            P = flat(model).numel()
            hd = None
            if ms.hd is not None:
                hd = torch.from_numpy(np.asarray(ms.hd if ms.entry == 'ensemble' else ms.hd[i], np.float64)).to(dev)
            want = run_single(dev, model.fused_desc(), model, ms.inputs[i], ms.ys[i], ms.bounds, ms.sched, ms.lrs[i], ham_diag=hd)
            for g, w, what in zip((params[i, :P], m1[i, :P], m2[i, :P], rows[i, :, :P + 2]), want, ('params', 'exp_avg',
                                                                                                     'exp_avg_sq', 'rows')):
                assert torch.equal(g, w), (i, what, float((g - w).abs().max()))
    finally:
        _lib.set_backward_variant('auto')


def run_variant(dev, ms, variant):
    from quanonet_amd import _lib
    _lib.set_backward_variant(variant)
    try:
        return ms.run(dev)
    finally:
        _lib.set_backward_variant('auto')


WORST = {}


def check_case(dev, cus, ms, name, bitwise=None, oracle_members=None):
    want = check_kernels(dev, cus, ms)
    got = ms.run(dev)
    WORST[name] = check_oracle(got, ms, oracle_members)
    print(f'worst-member-error {name} {WORST[name]:.2e}')
    if bitwise is not None:
        check_bitwise(dev, run_variant(dev, ms, bitwise), ms, bitwise)
    return want


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _hb(i):
    return (-1.0 - 0.25 * (i % 7), 1.0 + 0.5 * (i % 5))


# ---------------------------------------------------------------------------------------------------------------------
# edge cases: (id, entry, cells(cus), schedule(cus))
# ---------------------------------------------------------------------------------------------------------------------
UNROLLED = {2: (2, 2, 3, 2), 3: (2, 1, 2, 1), 4: (2, 2, 1, 2), 5: (2, 2, 1, 2)}


def _spw(n):
    return 64 >> lane_bits(n)


def _ens(n, net, R, **kw):
    return [cell(n, net, seed=s, **kw) for s in range(R)]


def _swp(n, net, R, **kw):
    return [cell(n, net, seed=s, hb=_hb(s), lr=1e-3 * (1 + s % 4), **kw) for s in range(R)]


def _short(nb):
    return [nb, max(1, (2 * nb) // 3)]


EDGE_CASES = []
for _n in (2, 3, 4, 5):
    for _lab, _k in (('C', 1), ('2C', 2), ('3C', 3)):
        # R x groups by R at a fixed batch of 8 sample groups per member (sweeps): k C and one member more
        for _d in (0, 1):
            EDGE_CASES.append((f'n{_n}-R-groups={_lab}{"+" if _d else ""}', 'sweep',
                               lambda c, n=_n, k=_k, d=_d: _swp(n, UNROLLED[n], k * c // 8 + d),
                               lambda c, n=_n: _short(8 * _spw(n))))
        # ... by the batch at R = 4 (ensembles): k C sample groups and one group more
        for _d in (0, 1):
            EDGE_CASES.append((f'n{_n}-B-groups={_lab}{"+1" if _d else ""}', 'ensemble',
                               lambda c, n=_n: _ens(n, UNROLLED[n], 4),
                               lambda c, n=_n, k=_k, d=_d: _short(k * c * _spw(n) // 4 + d)))


def _depth_edge(n):
    """QuanONet (1, D, 1, D) either side of the zpipes = 2 LDS limit (:624-627)"""
    D = 3
    while ztri2_lds(n, [(n, D + 1)] * 2) <= ZTRI2_LDS_LIMIT:
        D += 1
    return D


EDGE_CASES += [
    # odd sample-group counts per member under ztri<n, 2> (the last workgroup holds one pipeline)
    ('n5-odd-groups-ztri2', 'sweep', lambda c: _swp(5, UNROLLED[5], 3),
     lambda c: [2 * (2 * (c // 4) + 1) - 1, 2 * (2 * (c // 5) + 1) - 1]),
    ('n3-odd-groups-ztri2', 'ensemble', lambda c: _ens(3, UNROLLED[3], 3),
     lambda c: [8 * (2 * (c // 4) + 1) - 3, 8 * (2 * (c // 5) + 1) - 5]),
    # last zpacked workgroup of 1 and of kZPWaves - 1 = 3 sample groups (hea_zyz.hpp:1835) (the second with a partial sample group)
    ('n3-zpacked-last-1', 'sweep', lambda c: _swp(3, UNROLLED[3], 8), lambda c: [8 * (4 * (3 * c // 32) + 1), 8 * (4 * (3 * c // 32) + 1)]),
    ('n3-zpacked-last-3', 'ensemble', lambda c: _ens(3, UNROLLED[3], 8), lambda c: [8 * (4 * (3 * c // 32) + 3) - 5, 8 * (3 * c // 32 + 3)]),
    ('n2-zpacked-last-3', 'sweep', lambda c: _swp(2, UNROLLED[2], 5), lambda c: [16 * (4 * (3 * c // 20) + 3) - 1, 16 * 25 + 7]),
    # depths either side of the two-pipeline LDS limit (groups in (C, 2C])
    *[(f'n{n}-depth{D}', 'sweep', lambda c, n=n, D=D: _swp(n, (1, D, 1, D), 4), lambda c, n=n: _short(3 * c * _spw(n) // 8))
      for n in (5, 3) for D in (_depth_edge(n), _depth_edge(n) + 1)],
    # encoding width either side of the ZYZ table limit (n = 2: E <= 76): one grid / R calls in sequence
    ('n2-E76-grid', 'ensemble', lambda c: _ens(2, (19, 1, 19, 1), 3), lambda c: _short(100)),
    ('n2-E78-sequential', 'ensemble', lambda c: _ens(2, (20, 1, 19, 1), 3), lambda c: _short(100)),
    # a ragged shape (not block-unrolled) past 3 C: sequential, though each member alone would be pipelined
    ('n4-ragged-3C+-sequential', 'sweep', lambda c: _swp(4, (2, 1, 2, 2), 8), lambda c: _short(3 * c * 4 // 8 + 4)),
    # one step past 3 C sends the whole call to R calls in sequence (eligibility only grows as a step gets shorter, so the
    # ineligible step is the longer one); on a block-unrolled shape the shorter step only changes the kernel
    ('n4-ragged-one-step-sequential', 'ensemble', lambda c: _ens(4, (2, 1, 2, 2), 4), lambda c: [c, 3 * c + 4]),
    ('n4-unrolled-short-step-kernel', 'ensemble', lambda c: _ens(4, UNROLLED[4], 4), lambda c: [3 * c + 4, c]),
    # both sides of fused records (n = 2, one sub-layer per block: an even block count fuses), three steps
    ('n2-fused', 'ensemble', lambda c: _ens(2, (5, 1, 5, 1), 3), lambda c: [3000, 3000, 1200]),
    ('n2-not-fused', 'ensemble', lambda c: _ens(2, (5, 1, 4, 1), 3), lambda c: [3000, 3000, 1200]),
    ('n5-fused-zquad', 'sweep', lambda c: _swp(5, UNROLLED[5], 4), lambda c: [100, 100, 60]),
    # one Y member in a Z sweep at the zquad edge (groups = C): the all-lane ztri<5, 1>
    ('n5-Y-member-at-zquad-edge', 'sweep', lambda c: [x._replace(pauli='Y' if i == 2 else 'Z') for i, x in
                                                       enumerate(_swp(5, UNROLLED[5], 4))],
     lambda c: _short(2 * c // 4)),
    # R = 1 where the snapshot pipeline is chosen
    ('n5-R1-zsnap', 'ensemble', lambda c: _ens(5, UNROLLED[5], 1), lambda c: _short(3 * c)),
    ('n5-R1-sweep-zsnap', 'sweep', lambda c: _swp(5, UNROLLED[5], 1), lambda c: [3 * c, 3 * c]),
    # n = 7: R calls in sequence (status fold); n = 10: the workgroup-resident member grid
    ('n7-sequential', 'ensemble', lambda c: _ens(7, (1, 2, 1, 2), 3), lambda c: _short(100)),
    ('n7-sweep-sequential', 'sweep', lambda c: _swp(7, (1, 2, 1, 2), 3), lambda c: _short(100)),
    ('n10-lds-grid', 'ensemble', lambda c: _ens(10, (1, 1, 1, 1), 3), lambda c: _short(48)),
    ('n8-sequential-dense', 'sweep', lambda c: _swp(8, (1, 1, 1, 1), 2), lambda c: _short(4 * c + 1)),
    ('n10-R1-sequential', 'ensemble', lambda c: _ens(10, (1, 1, 1, 1), 1), lambda c: _short(48)),
    # R = 1: the single-model kernels on member 0's descriptor
    ('n3-R1-zpacked-ztri2', 'sweep', lambda c: _swp(3, UNROLLED[3], 1), lambda c: [3 * c * 8 + 8, c * 8 + 8]),
    ('n4-R1-ztri1', 'ensemble', lambda c: _ens(4, UNROLLED[4], 1), lambda c: [2 * c * 4 + 4, c * 4]),
    # R calls in sequence whose members take two pipelines, and the packed kernel (encoding too wide for the ZYZ table, each
    # member past 3 C)
    ('n4-ragged-sequential-ztri2', 'sweep', lambda c: _swp(4, (2, 1, 2, 2), 3), lambda c: [3 * c * 4 // 2, c * 4]),
    ('n2-E120-sequential-packed', 'ensemble', lambda c: _ens(2, (20, 1, 40, 1), 2), lambda c: [3 * c * 16 + 16, 8000]),
    # depth and qubit sweeps at n = 8, 9: R x waves = SIMDs and beyond (dense bwd_kernel)
    *[(f'depth-n{n}-waves={lab}', 'depth', lambda c, n=n: [cell(n, (1 + i % 2, 1, 1 + i // 2, 1), seed=i, lr=1e-3 * (1 + i))
                                                           for i in range(4)],
       lambda c, d=d: [c + d, c // 2]) for n in (8, 9) for lab, d in (('simd', 0), ('simd+', 1))],
    *[(f'qubit-n8n9-waves={lab}', 'qubit', lambda c: [cell(n, (1, 1, 1 + i % 2, 1), seed=i, lr=1e-3 * (1 + i))
                                                      for i, n in enumerate((8, 9, 8, 9, 3))],
       lambda c, d=d: [2 * c + d, c]) for lab, d in (('simd', 0), ('simd+', 1))],
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_member_edge_matches_oracle(dev, cus, case):
    name, entry, cells_f, sched_f = case
    ms = Members(entry, cells_f(cus), sched_f(cus), abs(hash(name)) % (1 << 31))
    check_case(dev, cus, ms, name)


# ---------------------------------------------------------------------------------------------------------------------
# past the fill chunks: R = 64, 65, 130 for each entry point, every member its own hyper-parameters
# ---------------------------------------------------------------------------------------------------------------------
def _spectrum(n, i):
    return np.sort(np.random.default_rng(1000 + i).uniform(-4, 4, size=1 << n))


def _chunk_cells(entry, R):
    if entry == 'ensemble':
        return _ens(3, (2, 2, 1, 2), R, scale=0.2)
    out = []
    for i in range(R):
        if entry == 'sweep':
            n, net = 3, (2, 2, 1, 2)
        elif entry == 'depth':
            n, net = 2, (1 + i % 5, 2, 1 + (i // 5) % 4, 2)
        else:
            n = (2, 3, 4, 5, 6, 7)[i % 6]
            net = (1 + i % 3, 2, 1 + (i // 3) % 2, 2)
        kw = dict(seed=i, lr=1e-3 * (1 + i % 7), scale=0.05 + 0.01 * (i % 11), trainable=False)
        if R == 65:                              # read-outs: Pauli Z / X / Y and bounds
            kw.update(pauli='ZXY'[i % 3], hb=_hb(i))
        else:                                    # a spectrum per member (Z read-outs)
            kw.update(diag=_spectrum(n, i))
        out.append(cell(n, net, **kw))
    return out


FORCED = {'ensemble': 'zpacked', 'sweep': 'zpacked', 'depth': 'packed', 'qubit': 'packed'}


@pytest.mark.gpu
@pytest.mark.parametrize('R', [64, 65, 130])
@pytest.mark.parametrize('entry', ['ensemble', 'sweep', 'depth', 'qubit'])
def test_past_the_fill_chunks(dev, cus, entry, R):
    ms = Members(entry, _chunk_cells(entry, R), [100, 37], 5000 + R)
    want = check_case(dev, cus, ms, f'{entry}-R{R}', bitwise=FORCED[entry])
    assert want.member_fills == -(-R // 64)


# the README's grids at their real size: synthetic data, 100 rows per step, two steps
def _grid_cells(runs):
    return [cell(n, (hb, 2, ht, 2), seed=s, scale=0.01, lr=1e-4) for n, hb, ht, s in runs]


CAPACITY = [(2, hb, ht, s) for hb in (50, 100, 150, 200) for ht in (10, 50, 100, 300) for s in range(5)]
SCALING = [(n, hb, ht, s) for n, (hbs, hts) in {2: ([50, 100, 150, 200], [10, 20, 30, 40, 50, 60, 100, 150, 200, 300]),
                                                 3: ([100, 200], [20, 40, 50, 100, 150, 200, 300]), 4: ([100, 200], [50, 100]),
                                                 5: ([100], [50, 100]), 6: ([100], [50, 100]), 7: ([100], [50, 100]),
                                                 8: ([100], [50, 100])}.items()
           for hb in hbs for ht in hts for s in range(5)]
CIRCUIT = [(n, hb, ht, s) for n, hbs in {2: [50, 100], 5: [20, 40], 10: [10, 20]}.items() for hb in hbs
           for ht in (10, 20, 30, 40) for s in range(5)]


@pytest.mark.gpu
@pytest.mark.parametrize('grid', ['capacity', 'scaling', 'circuit'])
def test_readme_grid_at_full_size(dev, cus, grid):
    runs, entry = {'capacity': (CAPACITY, 'depth'), 'scaling': (SCALING, 'qubit'), 'circuit': (CIRCUIT, 'qubit')}[grid]
    assert len(runs) == {'capacity': 80, 'scaling': 330, 'circuit': 120}[grid]
    ms = Members(entry, _grid_cells(runs), [100, 100], 6000 + len(runs), b_in=100, t_in=1)
    want = check_kernels(dev, cus, ms)
    assert want.member_fills == -(-len(runs) // 64)
    if grid == 'scaling':                        # list spread over the slices, class launches, one launch per n = 7, 8
        assert want.work_fills > 1 and [b[0] for b in want.bwd[:4]] == ['bwd_qsweep_kernel'] * 2 + ['bwd_kernel'] * 2
    got = run_variant(dev, ms, 'packed')
    check_bitwise(dev, got, ms, 'packed')
    # the oracle on every member; of the Q10 members of the circuit grid one seed per shape
    members = [i for i, (n, hb, ht, s) in enumerate(runs) if n < 10 or s == 0]
    auto = ms.run(dev)
    WORST[f'grid-{grid}'] = check_oracle(auto, ms, members)
    print(f'worst-member-error grid-{grid} {WORST[f"grid-{grid}"]:.2e}')


# ---------------------------------------------------------------------------------------------------------------------
# one solver: a 66-member SweepSolver against the PTSolver runs of members 0, 63, 64 and the last
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sweep_solver_past_one_fill_chunk(dev, tmp_path):
    from quanonet_amd.solver import PTSolver, set_random_seed
    from quanonet_amd.sweep import SweepSolver
    from tests.test_ensemble import _antideriv
    base = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'net_size': [5, 1, 5, 1], 'scale_coeff': 0.001,
            'if_trainable_freq': 'true', 'batch_size': 100, 'num_epochs': 1}
    cfgs = [dict(base, seed=i % 3, ham_bound=[-1.0 - i % 4, 1.0 + i % 5], learning_rate=1e-3 * (1 + i % 6), run_id=f'm{i}')
            for i in range(66)]
    data = _antideriv(250)
    quiet = lambda *a, **k: None
    sw = SweepSolver([dict(c, prefix=str(tmp_path / 'sweep')) for c in cfgs], data, device=dev, log=quiet)
    hists = sw.train()
    for i in (0, 63, 64, 65):
        c, h, m = cfgs[i], hists[i], sw.members[i]
        set_random_seed(c['seed'])
        solo = PTSolver(dict(c, prefix=str(tmp_path / 'solo')), data, device=dev, log=quiet)
        hs = solo.train()
        assert float((m.trainer.pflat.cpu() - solo.trainer.pflat.cpu()).abs().max()) < TOL, i
        assert np.allclose(h['loss_train'], hs['loss_train'], rtol=TOL, atol=0), i
        for f in ('best_model.pt', 'final.pt'):
            a, b = torch.load(os.path.join(m.out_dir, f)), torch.load(os.path.join(solo.out_dir, f))
            assert a.keys() == b.keys()
            for k in a:
                assert float((a[k] - b[k]).abs().max()) < TOL, (i, f, k)


# ---------------------------------------------------------------------------------------------------------------------
# coverage and the fixed points of the rules
# ---------------------------------------------------------------------------------------------------------------------
def _kind(r):
    """what a MemberRegime says, up to the qubit count: path, per backward launch its kernel, template arguments past n (pipes,
    dense build; the class of a class launch) and form; whether records are fused and whether the fills take several launches"""
    out = {('fused', r.path, r.fused > 0), ('fills', r.path, r.member_fills > 1, r.work_fills > 1)}
    for k, t, f, _ in r.bwd:
        out.add((r.path, k, (t if k == 'bwd_qsweep_kernel' else t[1:]) if t else None, f))
    return out


def _desc_of(c):
    from quanonet_amd import _lib
    net = list(c.net) if c.kind == 'QuanONet' else list(c.net[:2])
    return _lib.make_model_desc(_lib.MODEL_QUANONET if c.kind == 'QuanONet' else _lib.MODEL_HEAQNN, c.n, net, 6,
                                2 if c.kind == 'QuanONet' else 0, c.trainable, c.scale, 0.0, 1.0, c.pauli)


def _case_kinds(cus):
    out = set()
    for name, entry, cells_f, sched_f in EDGE_CASES:
        cells = cells_f(cus)
        out |= _kind(expected_member(entry, [_desc_of(c) for c in cells], len(cells), sched_f(cus), cus))
    for entry in ('ensemble', 'sweep', 'depth', 'qubit'):
        for R in (64, 65, 130):
            cells = _chunk_cells(entry, R)
            out |= _kind(expected_member(entry, [_desc_of(c) for c in cells], R, [100, 37], cus))
    for runs, entry in ((CAPACITY, 'depth'), (SCALING, 'qubit'), (CIRCUIT, 'qubit')):
        cells = _grid_cells(runs)
        out |= _kind(expected_member(entry, [_desc_of(c) for c in cells], len(cells), [100, 100], cus))
    return out


def _all_kinds(cus):
    """every kind expected_member returns over a sweep of entries, shapes, member counts, batches and read-outs (n <= 10)"""
    out = set()
    simd = 4 * cus
    for n in range(2, 11):
        shapes = [UNROLLED.get(n, (1, 2, 1, 2)), (2, 1, 2, 2), (1, 1, 1, 1)]
        if n <= 5:
            shapes.append((1, _depth_edge(n) + 1, 1, _depth_edge(n) + 1) if n in (3, 5) else (20, 1, 40, 1))
        spw = _spw(n)
        for net in shapes:
            for R in (1, 3, 8):
                for k in (0.25, 0.5, 1, 1.5, 2, 2.5, 3, 4, 6):
                    nb = max(1, int(k * cus * spw / R)) + 1
                    for sched in ([nb, nb, nb // 2 + 1], [nb // 2 + 1, nb]):
                        for pauli in ('Z', 'X'):
                            cells = [cell(n, net, pauli=pauli)] + [cell(n, net)] * (R - 1)
                            for entry in ('ensemble', 'sweep'):
                                ce = [cells[0]] * R if entry == 'ensemble' else cells
                                out |= _kind(expected_member(entry, [_desc_of(c) for c in ce], R, sched, cus))
        for R in (1, 4):
            for nb in (simd // R // 2, simd // R + 1):
                out |= _kind(expected_member('depth', [_desc_of(cell(n, (1, 1, 1, 1)))] * R, R, [nb], cus))
    for ns in ((2, 3), (2, 7), (3, 8, 8), (9, 9, 10)):
        for nb in (100, cus * 2 + 1):
            out |= _kind(expected_member('qubit', [_desc_of(cell(n, (1, 1, 1, 1))) for n in ns], len(ns), [nb], cus))
    for R in (3, 65):                            # fills of several launches
        for entry in ('ensemble', 'depth'):
            out |= _kind(expected_member(entry, [_desc_of(cell(3, (2, 2, 1, 2)))] * R, R, [100], cus))
        for net in ((1, 1, 1, 1), (200, 2, 300, 2)):
            out |= _kind(expected_member('qubit', [_desc_of(cell(2 + i % 6, net)) for i in range(R)], R, [100], cus))
    return out


@pytest.mark.gpu
def test_cases_cover_every_member_regime(cus):
    missing = _all_kinds(cus) - _case_kinds(cus)
    assert not missing, sorted(missing, key=str)


def _d(n, net, pauli='Z', kind='QuanONet'):
    return _desc_of(cell(n, net, pauli=pauli, kind=kind))


def test_expected_member_fixed_points():
    """the restated member rules at 256 CUs (MI355X): fixed points of the member table in DESIGN.md section 3.0"""
    c = CUS_NOMINAL
    u5, u3, rag4 = _d(5, (2, 2, 1, 2)), _d(3, (2, 1, 2, 1)), _d(4, (2, 1, 2, 2))
    # n = 5, 2 samples per group: R x groups = C -> zquad (member form), C + 1 -> ztri<5, 2>, 2C + 1 -> ztri<5, 1>,
    # 3C + 1 -> zpacked; never zsnap for R > 1, zsnap for R = 1 between C and 2C
    r = expected_member('ensemble', [u5] * 4, 4, [128, 100], c)
    assert r.path == 'grid' and r.bwd == (('bwd_zquad_kernel', None, 'ZBwdArgsM', 4), ('bwd_zquad_kernel', None, 'ZBwdArgsM', 4))
    assert r.member_fills == 1 and r.preps == 2 and r.folds == 0
    assert expected_member('ensemble', [u5] * 4, 4, [129], c).bwd == (('bwd_ztri_kernel', (5, 2), 'ZBwdArgsM', 4),)
    assert expected_member('ensemble', [u5] * 4, 4, [256], c).bwd == (('bwd_ztri_kernel', (5, 2), 'ZBwdArgsM', 4),)
    assert expected_member('ensemble', [u5] * 4, 4, [257], c).bwd == (('bwd_ztri_kernel', (5, 1), 'ZBwdArgsM', 4),)
    assert expected_member('ensemble', [u5] * 4, 4, [385], c).bwd == (('bwd_zpacked_kernel', (5,), 'ZBwdArgsM', 4),)
    assert expected_member('ensemble', [u5], 1, [768], c).bwd == (('bwd_zsnap_kernel', None, 'single', 1),)
    # a Y member: the all-lane kernels for the whole launch
    assert expected_member('sweep', [u5] * 3 + [_d(5, (2, 2, 1, 2), 'Y')], 4, [128], c).bwd[0][:2] == ('bwd_ztri_kernel', (5, 1))
    # fill launches: one per 64 members
    assert expected_member('sweep', [u3] * 65, 65, [100], c).member_fills == 2
    assert expected_member('sweep', [u3] * 130, 130, [100], c).member_fills == 3
    # a ragged shape beyond 3 C: R calls in sequence, each member's own (pipelined) regime, R - 1 status folds
    r = expected_member('sweep', [rag4] * 8, 8, [400, 200], c)
    assert r.path == 'sequential' and r.folds == 7 and r.member_fills == 0 and r.preps == 16
    assert set(r.bwd) == {('bwd_ztri_kernel', (4, 1), 'single', 1)}
    assert expected_member('sweep', [rag4] * 8, 8, [384, 200], c).path == 'grid'
    # one ineligible step: the whole call in sequence
    assert expected_member('ensemble', [rag4] * 4, 4, [256, 772], c).path == 'sequential'
    # fused records on the R x nb layout: n = 2, one sub-layer per block, even block count
    assert expected_member('ensemble', [_d(2, (5, 1, 5, 1))] * 3, 3, [3000, 3000, 1200], c).fused == 1
    assert expected_member('ensemble', [_d(2, (5, 1, 4, 1))] * 3, 3, [3000, 3000, 1200], c).fused == 0
    # the encoding width: n = 2, E = 76 grid, 78 sequential
    assert expected_member('ensemble', [_d(2, (19, 1, 19, 1))] * 3, 3, [100], c).path == 'grid'
    assert expected_member('ensemble', [_d(2, (20, 1, 19, 1))] * 3, 3, [100], c).path == 'sequential'
    # n = 7: sequential; n = 10: the depth grid's workgroup-resident member kernel
    assert expected_member('ensemble', [_d(7, (1, 2, 1, 2))] * 3, 3, [100], c).path == 'sequential'
    r = expected_member('ensemble', [_d(10, (1, 1, 1, 1))] * 3, 3, [48, 32], c)
    assert r.path == 'depth_grid' and r.bwd[0] == ('lds_bwd_kernel', (10,), 'DepthArgs', 3) and r.member_fills == 1
    # depth sweeps n = 8: dense iff R x nwaves > 1024
    d8 = [_d(8, (1, 1, 1, 1))] * 4
    assert expected_member('depth', d8, 4, [256], c).bwd == (('bwd_kernel', (8, 1), 'DepthArgs', 4),)
    assert expected_member('depth', d8, 4, [257], c).bwd == (('bwd_kernel', (8, 2), 'DepthArgs', 4),)
    assert expected_member('depth', [_d(2, (1, 1, 1, 1))] * 130, 130, [100], c).member_fills == 3
    # qubit sweeps: class launches, n = 8 / 9 launches with their member counts, work fills of 256 entries
    q = [_d(8, (1, 1, 1, 1)), _d(9, (1, 1, 1, 1))] * 2 + [_d(3, (1, 1, 1, 1))]
    r = expected_member('qubit', q, 5, [512, 256], c)
    assert r.bwd[:3] == (('bwd_qsweep_kernel', (3, 6, 1), 'class', 1), ('bwd_kernel', (8, 1), 'QubitArgs', 2),
                         ('bwd_kernel', (9, 1), 'QubitArgs', 2))
    assert expected_member('qubit', q, 5, [513], c).bwd[1] == ('bwd_kernel', (8, 2), 'QubitArgs', 2)
    r = expected_member('qubit', [_desc_of(x) for x in _grid_cells(SCALING)], 330, [100, 100], c)
    assert r.member_fills == 6 and r.work_fills > 1 and len(r.bwd) == 8
    assert [b[:2] for b in r.bwd[:4]] == [('bwd_qsweep_kernel', (2, 2, 1)), ('bwd_qsweep_kernel', (3, 6, 1)),
                                          ('bwd_kernel', (7, 1)), ('bwd_kernel', (8, 1))]
