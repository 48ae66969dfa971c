"""
Depth sweep (qhea_model_depth_sweep_train_steps, quanonet_amd.depth_sweep): what can be checked without a GPU -- the exported
symbols, which descriptor sets the workspace query accepts, Pmax against qhea_model_param_count, the argument checks that return
before anything is launched, and DepthSweepSolver's config validation (done before any device is touched).
"""
import ctypes
import math

import pytest

from quanonet_amd import _lib

QHEA_EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _q(hb, ht, n=2, bl=2, tl=2, b_in=10, t_in=1, trainable=True):
    return _lib.make_model_desc(_lib.MODEL_QUANONET, n, (hb, bl, ht, tl), b_in, t_in, trainable, 0.1, 0.0, 1.0)


def _h(depth, n=3, ld=2, x_in=4, trainable=True):
    return _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (depth, ld), x_in, 0, trainable, 0.1, 0.0, 1.0)


def test_depth_sweep_symbols_are_exported(lib):
    for name in ('qhea_model_depth_sweep_workspace_bytes', 'qhea_model_depth_sweep_train_steps'):
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert lib.qhea_version() >= 470


CAPACITY = [_q(hb, ht) for hb in (50, 100, 150, 200) for ht in (10, 50, 100, 300)]


@pytest.mark.parametrize('descs', [CAPACITY, [_q(5, 5), _q(40, 10), _q(60, 30)], [_q(3, 1, n=3), _q(1, 3, n=3)],
                                   [_q(2, 2, trainable=False), _q(7, 1, trainable=False)], [_h(1), _h(4), _h(9)],
                                   [_q(0, 4), _q(4, 0)], [_q(3, 3, n=10), _q(1, 2, n=10)]])
def test_depth_sweeps_of_depths_only_are_accepted(descs):
    assert _lib.model_depth_sweep_workspace_bytes(descs, 100) > 0


@pytest.mark.parametrize('other', [_q(5, 5, n=3), _q(5, 5, bl=1), _q(5, 5, tl=3), _q(5, 5, b_in=11), _q(5, 5, t_in=2),
                                   _q(5, 5, trainable=False), _h(5, n=2)])
def test_depth_sweeps_that_differ_elsewhere_are_rejected(lib, other):
    descs = [_q(5, 5), _q(10, 20), other]
    assert _lib.model_depth_sweep_workspace_bytes(descs, 100) == 0
    assert _call(lib, descs, [_m()] * 3) == QHEA_EINVAL


@pytest.mark.parametrize('other', [_h(3, n=4), _h(3, ld=1), _h(3, x_in=5), _h(3, trainable=False)])
def test_heaqnn_depth_sweeps_that_differ_elsewhere_are_rejected(other):
    assert _lib.model_depth_sweep_workspace_bytes([_h(2), other], 100) == 0


def test_pmax_and_member_counts_follow_param_count():
    counts = [_lib.model_param_count(d) for d in CAPACITY]
    assert _lib.depth_sweep_pmax(CAPACITY) == max(counts)
    # QuanONet, trainable frequency: bias + 2 (branch + trunk encoding columns) + 3 n sub-layers
    for d, p in zip(CAPACITY, counts):
        hb, bl, ht, tl = d.net
        E, blk = 2 * (hb + ht), hb * bl + ht * tl
        assert p == 1 + 2 * E + 3 * 2 * blk
    fixed = [_q(2, 2, trainable=False), _q(7, 1, trainable=False)]
    assert _lib.depth_sweep_pmax(fixed) == max(_lib.model_param_count(d) for d in fixed) == 1 + 3 * 2 * (7 * 2 + 2)


def test_workspace_covers_the_largest_member():
    small, big = _q(50, 10), _q(200, 300)
    ws = _lib.model_depth_sweep_workspace_bytes([small, big], 100)
    assert ws >= 2 * _lib.model_depth_sweep_workspace_bytes([big], 100) > 0
    assert ws == _lib.model_depth_sweep_workspace_bytes([big, small], 100)


def _m(pauli=0, lr=1e-3):
    m = _lib.MemberHParams(0.1, 0.0, 1.0, 1e-3, 0, 0)
    m.ham_pauli, m.lr = pauli, lr
    return m


def _call(lib, descs, members, n_models=None, diag=False, stride=None, steps=2):
    R = len(descs) if n_models is None else n_models
    arr = (_lib.ModelDesc * len(descs))(*descs)
    rb = (ctypes.c_int64 * 3)(0, 100, 150)
    ib = (ctypes.c_double * 2)(0.01, 0.02)
    fake = ctypes.c_void_p(4096)                # never dereferenced: every case fails its checks first
    mh = (_lib.MemberHParams * max(1, len(members)))(*members) if members is not None else None
    return lib.qhea_model_depth_sweep_train_steps(arr, R, mh, fake if diag else None, steps, rb, fake, fake, fake, fake, ib, fake,
                                                  _lib.depth_sweep_pmax(descs) + 2 if stride is None else stride, fake, fake, 1, 0.9, 0.999, 1e-8, 0.0,
                                                  fake, 1 << 30, None)


def test_depth_sweep_rejects_bad_arguments_before_launching(lib):
    descs = [_q(5, 5), _q(40, 10), _q(60, 30)]
    ms = [_m()] * 3
    assert _call(lib, descs, ms, n_models=0) == QHEA_EINVAL
    assert _call(lib, descs, ms, n_models=-1) == QHEA_EINVAL
    assert _call(lib, descs, None) == QHEA_EINVAL
    assert _call(lib, descs, ms, steps=0) == QHEA_EINVAL
    assert _call(lib, descs, [_m(), _m(), _m(pauli=3)]) == QHEA_EINVAL
    assert _call(lib, descs, [_m(), _m(pauli=1), _m()], diag=True) == QHEA_EINVAL
    for lr in (-1e-3, math.nan, math.inf):
        assert _call(lib, descs, [_m(), _m(lr=lr), _m()]) == QHEA_EINVAL, lr
    # a gradient row too short for the LARGEST member
    assert _call(lib, descs, ms, stride=_lib.depth_sweep_pmax(descs) + 1) == QHEA_EINVAL
    assert _call(lib, descs, ms, stride=_lib.model_param_count(descs[0]) + 2) == QHEA_EINVAL
    bad = _q(5, 5)
    bad.net[0] = -1
    assert _call(lib, [_q(5, 5), bad], [_m()] * 2, stride=1 << 20) == QHEA_EINVAL


BASE = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'net_size': [5, 2, 5, 2], 'scale_coeff': 0.001,
        'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': 100, 'num_epochs': 2, 'prefix': 'out'}


def _cfgs(**over):
    cs = [dict(BASE, seed=s, run_id=f'r{s}', net_size=[5 * (s + 1), 2, 10 * (s + 1), 2]) for s in range(3)]
    cs[2].update(over)
    return cs


@pytest.mark.parametrize('over', [dict(), dict(net_size=[200, 2, 300, 2]), dict(net_size=[1, 2, 0, 2]), dict(ham_pauli='X'),
                                  dict(learning_rate=1e-3), dict(operator='Other'), dict(ham_bound=[-2, 2])])
def test_depth_sweep_configs_may_differ_in_depths(over):
    from quanonet_amd.depth_sweep import validate_depth_sweep_configs
    cs = _cfgs(**over)
    assert validate_depth_sweep_configs(cs) == cs


def test_heaqnn_depth_sweep_configs():
    from quanonet_amd.depth_sweep import validate_depth_sweep_configs
    cs = [dict(BASE, model_type='HEAQNN', net_size=[d, 2], seed=0, run_id=f'd{d}') for d in (2, 4, 8)]
    assert validate_depth_sweep_configs(cs) == cs
    with pytest.raises(ValueError):
        validate_depth_sweep_configs(cs + [dict(BASE, model_type='HEAQNN', net_size=[2, 3], seed=0, run_id='ld3')])


@pytest.mark.parametrize('over', [dict(num_qubits=3), dict(net_size=[5, 1, 5, 2]), dict(net_size=[5, 2, 5, 3]),
                                  dict(net_size=[5, 2, 5]), dict(model_type='HEAQNN'), dict(if_trainable_freq='false'),
                                  dict(batch_size=50), dict(num_epochs=3), dict(run_id='r0'), dict(net_size=[-1, 2, 5, 2])])
def test_depth_sweep_rejects_configs_that_differ_elsewhere(over):
    from quanonet_amd.depth_sweep import validate_depth_sweep_configs
    with pytest.raises(ValueError):
        validate_depth_sweep_configs(_cfgs(**over))


@pytest.mark.parametrize('over', [dict(world_size=2), dict(epoch_call=False), dict(optimizer='sgd'), dict(num_qubits=3)])
def test_depth_sweep_solver_rejects_before_touching_a_device(over):
    import torch
    from quanonet_amd.depth_sweep import DepthSweepSolver
    with pytest.raises(ValueError):
        DepthSweepSolver(_cfgs(**over), {}, device=torch.device('cpu'))
