"""
The host side of the four quantum-jump gradient calls, recorded once and held (CPU, nothing is launched):
qhea_model_loss_grad_noisy_device / qhea_model_train_steps_noisy_device (n = 7..9) and their _lds forms (n = 10..12).

tests/golden/device_jump_grad_host_table.json holds what the library returned when the table was recorded
(tests/golden/make_device_jump_grad_host_table.py, with the library as it stood before the two units were given one host body);
the library under test must return the same.  Two parts:

  codes   the return code of every case: an otherwise good call with one defect, or two defects of different arguments, from
          DEFECTS.  The order in which a call reports what is wrong with its arguments is part of the ABI.  An empty batch or
          schedule counts as a defect: it ends the call with QHEA_OK once the checks in front of it have passed.  No case can
          reach a launch, whatever the library does with it: every call passes a NULL workspace, except the one-byte-short
          cases, which pass a non-NULL one of exactly one byte less than the size function asks for.
  sizes   the two workspace queries and qhea_noisy_device_lds_grad_max_workgroups on a grid: n = 6..13, both model kinds and a
          model whose blocks have no sub-layers, batch in BATCHES, T in TRAJECTORIES.  The work items of a launch, batch x
          ceil(T / tile), lie on both sides of every cap on the residents (2048 waves; 1024 / 512 / 256 workgroups), and T
          crosses a tile boundary of both tile sizes (4 and 2): the byte counts pin the layout's offsets and strides.
"""
import ctypes
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'device_jump_grad_host_table.json')

PTR = ctypes.c_void_p(0x1000)               # stands for a device pointer: the host never reads through one
ENTRIES = ('loss_grad_noisy_device', 'train_steps_noisy_device', 'loss_grad_noisy_device_lds', 'train_steps_noisy_device_lds')
LOSS_GRAD = ENTRIES[0::2]
STEPS = ENTRIES[1::2]
RANGE = {e: (10, 12) if e.endswith('_lds') else (7, 9) for e in ENTRIES}

# the pointers each call cannot do without (QuanONet's trunk apart)
REQUIRED = {e: ('branch', 'y', 'params', 'grad') if e in LOSS_GRAD else
            ('row_begin', 'inv_batch_total', 'branch', 'y', 'grad', 'params', 'exp_avg', 'exp_avg_sq') for e in ENTRIES}

MODELS = ((0, 'quanonet', [2, 1, 1, 2]), (1, 'heaqnn', [3, 2, 0, 0]))
QUBITS = range(6, 14)
BATCHES = (0, 1, 3, 600, 3000)
TRAJECTORIES = (1, 2, 5, 9)
SIZE_MODELS = MODELS + ((1, 'heaqnn_no_sublayers', [2, 0, 0, 0]),)
SIZE_FNS = ('qhea_model_noisy_device_grad_workspace_bytes', 'qhea_model_noisy_device_lds_grad_workspace_bytes')


def good_call(entry, model):
    """The arguments of a call that would run: model 0 = QuanONet, 1 = HEAQNN."""
    return dict(model=model, n=RANGE[entry][0] + 1, net=list(MODELS[model][2]), branch_in=3, trunk_in=2, trainable=1, pauli=0,
                null_desc=False, dn='ok', sampling=dict(shots=0, trajectories=5, seed=7),
                row0=0, batch=5, ham_diag=None, ws='null',
                branch=PTR, trunk=PTR, params=PTR, y=PTR, grad=PTR, exp_avg=PTR, exp_avg_sq=PTR,
                row_begin=[0, 3, 5, 10], inv_batch_total=[1 / 3, 1 / 2, 1 / 5], n_steps=3, first_step=1, grad_stride=1 << 20)


def device_noise_record(kind, n):
    """The qhea_device_noise of a case for n wires, or None: 'ok', 'null', 'p1_range' (a probability below 0), 'wires' (a record
    for another wire count), 'dead' (the last wire's CTL site has gamma = 1 in fp64: nothing to walk back through)"""
    from quanonet_amd.noise import DeviceNoise
    if kind == 'null':
        return None
    if kind == 'dead':
        return DeviceNoise(t1=[1.0] * (n - 1) + [1e-3], t2=[1.0] * (n - 1) + [1e-3], t_rx=0.001, t_rot=0.001, t_cx=0.1,
                           idle=False).params(n)
    rec = DeviceNoise(p1=0.01, p2=0.02, readout01=0.01, readout10=0.02, t1=50.0, t2=60.0, t_rx=0.02, t_rot=0.03,
                      t_cx=0.2).params(n - 1 if kind == 'wires' else n)
    if kind == 'p1_range':
        rec._arrays[0][0] = -0.1
    return rec


def _set(**kw):
    return lambda c: c.update(kw)


def _sampling(**kw):
    return lambda c: c['sampling'].update(kw) if c['sampling'] is not None else None


# name -> (the argument it spoils, the entry points it is a defect of (None: all), QuanONet only, what it does to the call)
DEFECTS = {
    'null_desc': ('desc', None, False, _set(null_desc=True)),
    'model_kind': ('model', None, False, _set(model=7)),
    'n_below': ('n', None, False, lambda c: c.update(n=c['n'] - 2)),                  # 6 / 9
    'n_above': ('n', None, False, lambda c: c.update(n=c['n'] + 2)),                  # 10 / 13
    'null_dn': ('dn', None, False, _set(dn='null')),
    'dn_p1_range': ('dn', None, False, _set(dn='p1_range')),
    'dn_wires': ('dn', None, False, _set(dn='wires')),
    'dn_gamma_1': ('dn', None, False, _set(dn='dead')),
    'null_sampling': ('sampling', None, False, _set(sampling=None)),
    'shot_mode': ('shots', None, False, _sampling(shots=3)),
    'T_0': ('trajectories', None, False, _sampling(trajectories=0)),
    'x_with_diag': ('pauli', None, False, lambda c: c.update(pauli=1, ham_diag=PTR)),
    'batch_negative': ('batch', LOSS_GRAD, False, _set(batch=-1)),
    'batch_0': ('batch', LOSS_GRAD, False, _set(batch=0)),
    'batch_overflow': ('batch', LOSS_GRAD, False, _set(batch=1 << 31)),               # rows x tiles past INT_MAX
    'row0_negative': ('row0', LOSS_GRAD, False, _set(row0=-1)),
    'no_trunk': ('trunk', None, True, _set(trunk=None)),
    'ws_null': ('ws', None, False, _set(ws='null')),
    'ws_short': ('ws', None, False, _set(ws='short')),
    'first_step_0': ('first_step', STEPS, False, _set(first_step=0)),
    'n_steps_negative': ('n_steps', STEPS, False, _set(n_steps=-1)),
    'n_steps_0': ('n_steps', STEPS, False, _set(n_steps=0)),
    'row_begin_decreasing': ('row_begin', STEPS, False, _set(row_begin=[0, 5, 3, 10])),
    'row_begin_overflow': ('row_begin', STEPS, False, _set(row_begin=[0, 3, 5, 5 + (1 << 31)])),
    'grad_stride_short': ('grad_stride', STEPS, False, _set(grad_stride=3)),
}
for _e in ENTRIES:
    for _p in REQUIRED[_e]:
        DEFECTS.setdefault(f'null_{_p}', (_p, [], False, _set(**{_p: None})))[1].append(_e)


def cases(entry, model):
    """(names) of every single defect and every pair of defects of different arguments that applies to the call"""
    names = [k for k, (_, where, quanonet, _f) in DEFECTS.items() if (where is None or entry in where) and (not quanonet or model == 0)]
    out = [(k,) for k in names]
    out += [(a, b) for a, b in itertools.combinations(names, 2) if DEFECTS[a][0] != DEFECTS[b][0]]
    return out


def spoiled_call(entry, model, names):
    c = good_call(entry, model)
    for k in names:
        DEFECTS[k][3](c)
    return c


def run_case(lib, entry, c):
    """The call's return code.  Only ws_short passes a workspace, of one byte less than the size function's answer."""
    from quanonet_amd import _lib
    desc = None
    if not c['null_desc']:
        desc = ctypes.byref(_lib.ModelDesc(c['model'], c['n'], (ctypes.c_int32 * 4)(*c['net']), c['branch_in'], c['trunk_in'],
                                           c['trainable'], c['pauli'], 0.1, 0.0, 1.0))
    rec = device_noise_record(c['dn'], c['n'])
    dn = None if rec is None else ctypes.byref(rec)
    sp = c['sampling']
    sampling = None if sp is None else ctypes.byref(_lib.SamplingParams(sp['shots'], sp['trajectories'], sp['seed']))
    rb = c['row_begin'] and (ctypes.c_int64 * len(c['row_begin']))(*c['row_begin'])
    ib = c['inv_batch_total'] and (ctypes.c_double * len(c['inv_batch_total']))(*c['inv_batch_total'])
    rows = c['batch'] if entry in LOSS_GRAD else max([b - a for a, b in zip(c['row_begin'], c['row_begin'][1:])] if rb else [0])
    total = getattr(lib, SIZE_FNS[entry.endswith('_lds')])(desc, rows, sampling)
    ws, ws_bytes = (PTR, total - 1) if c['ws'] == 'short' and total > 0 else (None, 0)
    assert ws is None or ws_bytes < total                # (what keeps every case in front of the first launch)
    fn = getattr(lib, f'qhea_model_{entry}')
    if entry in LOSS_GRAD:
        return fn(desc, c['row0'], c['batch'], c['branch'], c['trunk'], c['y'], c['params'], c['ham_diag'], dn, sampling, 0.2,
                  c['grad'], None, ws, ws_bytes, None)
    return fn(desc, c['n_steps'], rb or None, c['branch'], c['trunk'], c['y'], c['params'], c['ham_diag'], dn, sampling, ib or None,
              c['grad'], c['grad_stride'], c['exp_avg'], c['exp_avg_sq'], c['first_step'], 1e-3, 0.9, 0.999, 1e-8, 0.0, ws,
              ws_bytes, None)


def all_codes(lib):
    """{'entry/model': {'defect+defect': code}} over the whole table"""
    out = {}
    for entry in ENTRIES:
        for model, tag, _net in MODELS:
            out[f'{entry}/{tag}'] = {'+'.join(names): run_case(lib, entry, spoiled_call(entry, model, names))
                                     for names in cases(entry, model)}
    return out


def all_sizes(lib):
    """{'size function/model': {'n=..,B=..,T=..': bytes}} over the grid, and {'max_workgroups': {'n': count}}"""
    from quanonet_amd import _lib
    out = {'max_workgroups': {str(n): lib.qhea_noisy_device_lds_grad_max_workgroups(n) for n in QUBITS}}
    for fn in SIZE_FNS:
        for model, tag, net in SIZE_MODELS:
            col = out[f'{fn}/{tag}'] = {}
            for n, B, T in itertools.product(QUBITS, BATCHES, TRAJECTORIES):
                desc = _lib.ModelDesc(model, n, (ctypes.c_int32 * 4)(*net), 3, 2, 1, 0, 0.1, 0.0, 1.0)
                col[f'n={n},B={B},T={T}'] = getattr(lib, fn)(ctypes.byref(desc), B, ctypes.byref(_lib.SamplingParams(0, T, 7)))
    return out


def all_tables(lib):
    return {'codes': all_codes(lib), 'sizes': all_sizes(lib)}


@pytest.fixture(scope='module')
def tables():
    from quanonet_amd import _lib
    return all_tables(_lib.load())


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_covers_the_issue_list():
    """every defect is a case of some call, every call has its singles and pairs, and every case carries a defect"""
    used = set()
    for entry in ENTRIES:
        for model, _tag, _net in MODELS:
            cs = cases(entry, model)
            assert all(1 <= len(names) <= 2 for names in cs)
            singles = {names[0] for names in cs if len(names) == 1}
            assert {'null_desc', 'null_dn', 'dn_p1_range', 'null_sampling', 'shot_mode', 'T_0', 'n_below', 'n_above', 'dn_gamma_1',
                    'ws_null', 'ws_short'} <= singles
            assert {f'null_{p}' for p in REQUIRED[entry]} <= singles
            assert ({'first_step_0', 'n_steps_negative', 'n_steps_0', 'row_begin_overflow'} <= singles) == (entry in STEPS)
            assert ({'batch_0', 'batch_overflow'} <= singles) == (entry in LOSS_GRAD)
            assert ('no_trunk' in singles) == (model == 0)
            pairs = {frozenset(names) for names in cs if len(names) == 2}
            assert all(frozenset((a, b)) in pairs or DEFECTS[a][0] == DEFECTS[b][0] for a, b in itertools.combinations(singles, 2))
            used |= singles
    assert used == set(DEFECTS)


def test_grid_lies_on_both_sides_of_every_cap(golden):
    """the items of the grid against the caps the recorded table itself states, and a tile boundary inside T for both tiles"""
    caps = [2048] + [golden['sizes']['max_workgroups'][str(n)] for n in (10, 11, 12)]
    assert caps[1:] == [1024, 512, 256]
    for tile, unit_caps in ((4, caps[:1]), (2, caps[1:])):
        tiles = sorted({-(-T // tile) for T in TRAJECTORIES})
        assert len(tiles) > 1
        items = {B * t for B in BATCHES for t in tiles}
        for cap in unit_caps:
            assert any(0 < i < cap for i in items) and any(i > cap for i in items)


@pytest.mark.parametrize('entry', ENTRIES)
def test_return_codes_as_recorded(tables, golden, entry):
    for _model, tag, _net in MODELS:
        got, want = tables['codes'][f'{entry}/{tag}'], golden['codes'][f'{entry}/{tag}']
        assert sorted(got) == sorted(want), "the case table and the recorded table differ: record again"
        diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
        assert not diff, f"{entry}/{tag}: (returned, recorded) {diff}"


def test_sizes_as_recorded(tables, golden):
    got, want = tables['sizes'], golden['sizes']
    assert sorted(got) == sorted(want), "the grid and the recorded table differ: record again"
    for key in got:
        assert sorted(got[key]) == sorted(want[key]), "the grid and the recorded table differ: record again"
        diff = {k: (got[key][k], want[key][k]) for k in got[key] if got[key][k] != want[key][k]}
        assert not diff, f"{key}: (returned, recorded) {diff}"


def test_recorded_table_is_the_documented_one(golden):
    """a few entries of the recorded table itself, against what the header documents"""
    ok, inval, unsupported, workspace = 0, -1, -2, -3
    g = golden['codes']
    for entry in ENTRIES:
        for tag in ('quanonet', 'heaqnn'):
            t = g[f'{entry}/{tag}']
            assert t['ws_null'] == workspace and t['ws_short'] == workspace
            assert t['null_desc'] == inval and t['null_dn'] == inval and t['null_sampling'] == inval and t['shot_mode'] == inval
            assert t['T_0'] == inval and t['dn_gamma_1'] == inval and t['dn_p1_range'] == inval
            # (13 qubits is no descriptor at all)
            assert t['n_below'] == unsupported and t['n_above'] == (inval if entry.endswith('_lds') else unsupported)
            assert t['n_below+dn_p1_range'] == inval                  # the device-noise record before the qubit range
            assert t['n_below+x_with_diag'] == unsupported            # the qubit range before the read-out
            assert t['dn_gamma_1+ws_short'] == inval                  # the site that cannot be walked back before the workspace
    for entry in LOSS_GRAD:
        t = g[f'{entry}/heaqnn']
        assert t['batch_0'] == ok and t['batch_0+ws_short'] == ok
        assert t['shot_mode+batch_0'] == inval and t['dn_gamma_1+batch_0'] == inval     # the setting's checks are the call's
        assert t['batch_overflow'] == workspace
    for entry in STEPS:
        t = g[f'{entry}/quanonet']
        assert t['n_steps_0'] == ok and t['null_desc+n_steps_0'] == inval and t['first_step_0+n_steps_0'] == inval
        assert t['n_steps_negative'] == inval and t['row_begin_decreasing'] == inval and t['row_begin_overflow'] == workspace
    s = golden['sizes']
    for fn, (lo, hi) in zip(SIZE_FNS, ((7, 9), (10, 12))):
        for _model, tag, _net in SIZE_MODELS:
            for n, B, T in itertools.product(QUBITS, BATCHES, TRAJECTORIES):
                assert (s[f'{fn}/{tag}'][f'n={n},B={B},T={T}'] > 0) == (lo <= n <= hi)
