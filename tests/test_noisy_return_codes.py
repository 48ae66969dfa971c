"""
Return codes of the five noisy entry points, recorded once and held (CPU, nothing is launched).

The order in which a call reports what is wrong with its arguments is part of the ABI: a bad noise setting before the qubit
range, the conditioning of a gradient call after its read-out, a short workspace last.  tests/golden/noisy_return_codes.json
holds the code every case below returned when the table was recorded (tests/golden/make_noisy_return_codes.py, with the
library as it stood before the five calls were given one shared preamble); the library under test must return the same.

A case is an otherwise good call with one defect, or two defects of different arguments, from DEFECTS.  An empty batch or
schedule counts as one: it ends the call with QHEA_OK before anything else is looked at.  No case can reach a launch,
whatever the library does with it: every call passes a NULL workspace, except the one-byte-short cases, which pass a
non-NULL one of exactly one byte less than the size function asks for.
"""
import ctypes
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'noisy_return_codes.json')

PTR = ctypes.c_void_p(0x1000)               # stands for a device pointer: the host never reads through one
ENTRIES = ('forward_noisy', 'forward_noisy_wide', 'forward_noisy_exact', 'loss_grad_noisy_exact', 'train_steps_noisy_exact')
TRAJ = ENTRIES[:2]
GRAD = ENTRIES[3:]
STEPS = ENTRIES[4]

# the pointers each call cannot do without (QuanONet's trunk apart)
REQUIRED = {
    'forward_noisy': ('branch', 'params', 'pred'),
    'forward_noisy_wide': ('branch', 'params', 'pred'),
    'forward_noisy_exact': ('branch', 'params', 'pred'),
    'loss_grad_noisy_exact': ('branch', 'y', 'params', 'grad'),
    'train_steps_noisy_exact': ('row_begin', 'inv_batch_total', 'branch', 'y', 'grad', 'params', 'exp_avg', 'exp_avg_sq'),
}


def good_call(entry, model):
    """The arguments of a call that would run: model 0 = QuanONet, 1 = HEAQNN."""
    wide = entry == 'forward_noisy_wide'
    c = dict(model=model, n=8 if wide else 3, net=[2, 1, 1, 2] if model == 0 else [3, 2, 0, 0], branch_in=3, trunk_in=2,
             trainable=1, pauli=0, null_desc=False,
             noise=dict(p1=0.01, p2=0.02, readout=0.03, shots=0, trajectories=150, seed=7),
             row0=0, batch=5, ham_diag=None, ws='null',
             branch=PTR, trunk=PTR, params=PTR, pred=PTR, y=PTR, grad=PTR, exp_avg=PTR, exp_avg_sq=PTR,
             row_begin=[0, 3, 5, 10], inv_batch_total=[1 / 3, 1 / 2, 1 / 5], n_steps=3, first_step=1, grad_stride=1 << 20)
    return c


def _set(**kw):
    return lambda c: c.update(kw)


def _noise(**kw):
    return lambda c: c['noise'].update(kw) if c['noise'] is not None else None


def _x_with_diag(c):
    c.update(pauli=1, ham_diag=PTR)


# name -> (the argument it spoils, the entry points it is a defect of (None: all), QuanONet only, what it does to the call)
DEFECTS = {
    'null_desc': ('desc', None, False, _set(null_desc=True)),
    'model_kind': ('model', None, False, _set(model=7)),
    'net_negative': ('net', None, False, lambda c: c['net'].__setitem__(1, -1)),
    'branch_in_0': ('branch_in', None, False, _set(branch_in=0)),
    'pauli_code': ('pauli', None, False, _set(pauli=3)),
    'n_1': ('n', None, False, _set(n=1)),
    'n_13': ('n', None, False, _set(n=13)),
    'n_other_side': ('n', None, False, lambda c: c.update(n=6 if c['n'] == 8 else 7)),
    'null_noise': ('noise', None, False, _set(noise=None)),
    'p1_range': ('p1', None, False, _noise(p1=-0.01)),
    'p2_range': ('p2', None, False, _noise(p2=1.5)),
    'readout_range': ('readout', None, False, _noise(readout=2.0)),
    'p1_nan': ('p1', None, False, _noise(p1=float('nan'))),
    'shots_negative': ('shots', TRAJ, False, _noise(shots=-3)),
    'T_0': ('trajectories', TRAJ, False, _noise(trajectories=0)),
    'T_2^32': ('trajectories', TRAJ, False, _noise(trajectories=1 << 32)),
    'x_with_diag': ('pauli', None, False, _x_with_diag),
    'batch_negative': ('batch', ENTRIES[:4], False, _set(batch=-1)),
    'batch_0': ('batch', ENTRIES[:4], False, _set(batch=0)),
    'row0_negative': ('row0', TRAJ, False, _set(row0=-1)),
    'no_trunk': ('trunk', None, True, _set(trunk=None)),
    'ws_null': ('ws', None, False, _set(ws='null')),
    'ws_short': ('ws', None, False, _set(ws='short')),
    'first_step_0': ('first_step', (STEPS,), False, _set(first_step=0)),
    'n_steps_negative': ('n_steps', (STEPS,), False, _set(n_steps=-1)),
    'n_steps_0': ('n_steps', (STEPS,), False, _set(n_steps=0)),
    'row_begin_decreasing': ('row_begin', (STEPS,), False, _set(row_begin=[0, 5, 3, 10])),
    'row_begin_negative': ('row_begin', (STEPS,), False, _set(row_begin=[-2, 3, 5, 10])),
    'grad_stride_short': ('grad_stride', (STEPS,), False, _set(grad_stride=3)),
    'amplification': ('p1', GRAD, False, _noise(p1=0.7)),
    'singular_channel': ('p1', GRAD, False, _noise(p1=0.75)),
}
for _e in ENTRIES:
    for _p in REQUIRED[_e]:
        DEFECTS.setdefault(f'null_{_p}', (_p, [], False, _set(**{_p: None})))[1].append(_e)


def cases(entry, model):
    """(id, names) of every single defect and every pair of defects of different arguments that applies to the call"""
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
    nz = c['noise']
    noise = None if nz is None else ctypes.byref(_lib.NoiseParams(nz['p1'], nz['p2'], nz['readout'], nz['shots'],
                                                                  nz['trajectories'], nz['seed']))
    rb = c['row_begin'] and (ctypes.c_int64 * len(c['row_begin']))(*c['row_begin'])
    ib = c['inv_batch_total'] and (ctypes.c_double * len(c['inv_batch_total']))(*c['inv_batch_total'])
    rows = c['batch'] if entry != STEPS else max([b - a for a, b in zip(c['row_begin'], c['row_begin'][1:])] if rb else [0])
    if entry in TRAJ:
        tag = 'noisy_wide' if entry == 'forward_noisy_wide' else 'noisy'
        total = getattr(lib, f'qhea_model_{tag}_workspace_bytes')(desc, rows, noise)
    elif entry == 'forward_noisy_exact':
        total = lib.qhea_model_exact_noisy_workspace_bytes(desc, rows)
    else:
        total = lib.qhea_model_exact_noisy_grad_workspace_bytes(desc, rows)
    ws, ws_bytes = (PTR, total - 1) if c['ws'] == 'short' and total > 0 else (None, 0)
    assert ws is None or ws_bytes < total                # (what keeps every case in front of the first launch)
    fn = getattr(lib, f'qhea_model_{entry}')
    if entry in TRAJ:
        return fn(desc, c['row0'], c['batch'], c['branch'], c['trunk'], c['params'], c['ham_diag'], noise, c['pred'], None, ws,
                  ws_bytes, None)
    if entry == 'forward_noisy_exact':
        return fn(desc, c['batch'], c['branch'], c['trunk'], c['params'], c['ham_diag'], noise, c['pred'], None, ws, ws_bytes, None)
    if entry == 'loss_grad_noisy_exact':
        return fn(desc, c['batch'], c['branch'], c['trunk'], c['y'], c['params'], c['ham_diag'], noise, 0.2, c['grad'], None, ws,
                  ws_bytes, None)
    return fn(desc, c['n_steps'], rb or None, c['branch'], c['trunk'], c['y'], c['params'], c['ham_diag'], noise, ib or None,
              c['grad'], c['grad_stride'], c['exp_avg'], c['exp_avg_sq'], c['first_step'], 1e-3, 0.9, 0.999, 1e-8, 0.0, ws,
              ws_bytes, None)


def all_codes(lib):
    """{'entry/model': {'defect+defect': code}} over the whole table"""
    out = {}
    for entry in ENTRIES:
        for model, tag in ((0, 'quanonet'), (1, 'heaqnn')):
            out[f'{entry}/{tag}'] = {'+'.join(names): run_case(lib, entry, spoiled_call(entry, model, names))
                                     for names in cases(entry, model)}
    return out


@pytest.fixture(scope='module')
def codes():
    from quanonet_amd import _lib
    return all_codes(_lib.load())


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_covers_the_issue_list():
    """every defect is a case of some call, every call has its singles and pairs, and every case carries a defect"""
    used = set()
    for entry in ENTRIES:
        for model in (0, 1):
            cs = cases(entry, model)
            assert all(1 <= len(names) <= 2 for names in cs)
            singles = {names[0] for names in cs if len(names) == 1}
            assert {'null_desc', 'n_1', 'n_13', 'n_other_side', 'null_noise', 'p1_range', 'p2_range', 'readout_range', 'x_with_diag',
                    'ws_null', 'ws_short'} <= singles
            assert {f'null_{p}' for p in REQUIRED[entry]} <= singles
            assert ('no_trunk' in singles) == (model == 0)
            pairs = {frozenset(names) for names in cs if len(names) == 2}
            assert all(frozenset((a, b)) in pairs or DEFECTS[a][0] == DEFECTS[b][0] for a, b in itertools.combinations(singles, 2))
            used |= singles
    assert used == set(DEFECTS)


@pytest.mark.parametrize('entry', ENTRIES)
def test_return_codes_as_recorded(codes, golden, entry):
    for tag in ('quanonet', 'heaqnn'):
        got, want = codes[f'{entry}/{tag}'], golden[f'{entry}/{tag}']
        assert sorted(got) == sorted(want), "the case table and the recorded table differ: record again"
        diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
        assert not diff, f"{entry}/{tag}: (returned, recorded) {diff}"


def test_recorded_order_is_the_documented_one(golden):
    """a few entries of the recorded table itself, against the order the header documents"""
    inval, unsupported, workspace = -1, -2, -3
    g = golden
    assert g['forward_noisy/heaqnn']['n_other_side+p1_range'] == inval             # noise setting before the qubit range
    assert g['forward_noisy_wide/heaqnn']['n_other_side+p1_range'] == inval
    assert g['forward_noisy/heaqnn']['n_other_side+x_with_diag'] == unsupported    # qubit range before the read-out
    assert g['loss_grad_noisy_exact/heaqnn']['x_with_diag+amplification'] == inval  # conditioning after the read-out
    assert g['loss_grad_noisy_exact/heaqnn']['batch_negative+amplification'] == unsupported
    assert g['train_steps_noisy_exact/quanonet']['null_desc+n_steps_0'] == inval
    assert g['train_steps_noisy_exact/quanonet']['first_step_0+singular_channel'] == inval
    assert g['train_steps_noisy_exact/quanonet']['n_steps_0+singular_channel'] == unsupported
    assert g['train_steps_noisy_exact/quanonet']['ws_short'] == workspace
    for entry in ENTRIES[:4]:
        assert g[f'{entry}/quanonet']['batch_0+ws_short'] == 0 and g[f'{entry}/quanonet']['ws_null'] == workspace
