"""
Qubit sweep (qhea_model_qubit_sweep_train_steps, quanonet_amd.qubit_sweep): what can be checked without a GPU -- the exported
symbols, which descriptor sets the workspace query accepts and its size, the argument checks that return before anything is
launched, and QubitSweepSolver's config validation (done before any device is touched).
"""
import ctypes

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


def test_qubit_sweep_symbols_are_exported(lib):
    for name in ('qhea_model_qubit_sweep_workspace_bytes', 'qhea_model_qubit_sweep_train_steps'):
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert lib.qhea_version() >= 480


# reproduce_scaling.sh-shaped: Q2..Q8, each with its own depths
SCALING = [_q(hb, ht, n=n) for n, (hb, ht) in zip(range(2, 9), ((20, 10), (10, 5), (8, 4), (5, 3), (4, 2), (3, 2), (2, 1)))]


@pytest.mark.parametrize('descs', [SCALING, [_q(5, 5, n=2), _q(5, 5, n=9)], [_q(3, 1, n=3), _q(1, 3, n=7), _q(2, 2, n=10)],
                                   [_q(2, 2, n=4, trainable=False), _q(7, 1, n=8, trainable=False)],
                                   [_h(1, n=2), _h(4, n=5), _h(2, n=9)], [_q(0, 4, n=6), _q(4, 0, n=3)], [_q(1, 1, n=12)]])
def test_qubit_sweeps_of_qubit_counts_and_depths_are_accepted(descs):
    assert _lib.model_qubit_sweep_workspace_bytes(descs, 100) > 0


@pytest.mark.parametrize('other', [_q(5, 5, n=3, bl=1), _q(5, 5, n=4, tl=3), _q(5, 5, n=5, b_in=11), _q(5, 5, n=6, t_in=2),
                                   _q(5, 5, n=3, trainable=False), _h(5, n=2)])
def test_qubit_sweeps_that_differ_elsewhere_are_rejected(lib, other):
    descs = [_q(5, 5), _q(10, 20, n=5), other]
    assert _lib.model_qubit_sweep_workspace_bytes(descs, 100) == 0
    assert _call(lib, descs, [_m()] * 3) == QHEA_EINVAL


@pytest.mark.parametrize('other', [_h(3, n=4, ld=1), _h(3, n=5, x_in=5), _h(3, n=2, trainable=False)])
def test_heaqnn_qubit_sweeps_that_differ_elsewhere_are_rejected(other):
    assert _lib.model_qubit_sweep_workspace_bytes([_h(2), other], 100) == 0


@pytest.mark.parametrize('n', [1, 13])
def test_qubit_counts_out_of_range_are_rejected(lib, n):
    descs = [_q(2, 2), _q(2, 2, n=n)]
    assert _lib.model_qubit_sweep_workspace_bytes(descs, 100) == 0
    assert _call(lib, descs, [_m()] * 2, stride=1 << 20) == QHEA_EINVAL


def test_workspace_is_r_slices_each_covering_the_largest_member():
    for batch in (1, 37, 100, 1000):
        ws = _lib.model_qubit_sweep_workspace_bytes(SCALING, batch)
        R = len(SCALING)
        assert ws > 0 and ws % R == 0
        # a slice holds every member's own depth-sweep slice
        biggest = max(_lib.model_depth_sweep_workspace_bytes([d], batch) for d in SCALING)
        assert ws // R >= biggest
        assert ws == _lib.model_qubit_sweep_workspace_bytes(SCALING[::-1], batch)
    small = _lib.model_qubit_sweep_workspace_bytes(SCALING, 100)
    assert _lib.model_qubit_sweep_workspace_bytes(SCALING, 1000) > small
    # with an n >= 10 member the slice also holds its single-model layout
    mixed = [_q(2, 2, n=3), _q(2, 2, n=10)]
    assert _lib.model_qubit_sweep_workspace_bytes(mixed, 100) // 2 >= _lib.model_depth_sweep_workspace_bytes([mixed[1]], 100)
    assert _lib.model_qubit_sweep_workspace_bytes([_q(5, 5)], 100) > 0
    assert _lib.model_qubit_sweep_workspace_bytes(SCALING, -1) == 0


def test_pmax_is_the_largest_member():
    assert _lib.qubit_sweep_pmax(SCALING) == max(_lib.model_param_count(d) for d in SCALING)


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
    return lib.qhea_model_qubit_sweep_train_steps(arr, R, mh, fake if diag else None, steps, rb, fake, fake, fake, fake, ib, fake,
                                                  _lib.qubit_sweep_pmax(descs) + 2 if stride is None else stride, fake, fake, 1,
                                                  0.9, 0.999, 1e-8, 0.0, fake, 1 << 30, None)


def test_qubit_sweep_rejects_bad_arguments_before_launching(lib):
    descs = [_q(5, 5), _q(4, 10, n=5), _q(2, 3, n=8)]
    ms = [_m()] * 3
    assert _call(lib, descs, ms, n_models=0) == QHEA_EINVAL
    assert _call(lib, descs, None) == QHEA_EINVAL
    assert _call(lib, descs, ms, steps=0) == QHEA_EINVAL
    assert _call(lib, descs, [_m(), _m(), _m(pauli=3)]) == QHEA_EINVAL
    assert _call(lib, descs, [_m(), _m(pauli=1), _m()], diag=True) == QHEA_EINVAL
    assert _call(lib, descs, [_m(), _m(lr=-1.0), _m()]) == QHEA_EINVAL
    assert _call(lib, descs, ms, stride=_lib.qubit_sweep_pmax(descs) + 1) == QHEA_EINVAL


BASE = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'net_size': [5, 2, 5, 2], 'scale_coeff': 0.001,
        'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': 100, 'num_epochs': 2, 'prefix': 'out'}


def _cfgs(**over):
    cs = [dict(BASE, seed=s, run_id=f'r{s}', num_qubits=2 + 3 * s, net_size=[5 * (s + 1), 2, 2 * (s + 1), 2]) for s in range(3)]
    cs[2].update(over)
    return cs


@pytest.mark.parametrize('over', [dict(), dict(num_qubits=12), dict(num_qubits=3, net_size=[1, 2, 0, 2]), dict(ham_pauli='X'),
                                  dict(learning_rate=1e-3)])
def test_qubit_sweep_configs_may_differ_in_qubits_and_depths(over):
    from quanonet_amd.qubit_sweep import validate_qubit_sweep_configs
    cs = _cfgs(**over)
    assert validate_qubit_sweep_configs(cs) == cs


def test_heaqnn_qubit_sweep_configs():
    from quanonet_amd.qubit_sweep import validate_qubit_sweep_configs
    cs = [dict(BASE, model_type='HEAQNN', num_qubits=n, net_size=[d, 2], seed=0, run_id=f'q{n}d{d}')
          for n, d in ((2, 2), (5, 4), (9, 1))]
    assert validate_qubit_sweep_configs(cs) == cs
    with pytest.raises(ValueError):
        validate_qubit_sweep_configs(cs + [dict(BASE, model_type='HEAQNN', num_qubits=3, net_size=[2, 3], seed=0, run_id='ld3')])


@pytest.mark.parametrize('over', [dict(net_size=[5, 1, 5, 2]), dict(net_size=[5, 2, 5, 3]), dict(model_type='HEAQNN'),
                                  dict(if_trainable_freq='false'), dict(num_qubits=1), dict(num_qubits=0),
                                  dict(num_qubits=3, ham_diag=[0.0, 1.0, 2.0, 3.0]), dict(batch_size=50), dict(run_id='r0'),
                                  dict(net_size=[-1, 2, 5, 2])])
def test_qubit_sweep_rejects_configs_that_differ_elsewhere(over):
    from quanonet_amd.qubit_sweep import validate_qubit_sweep_configs
    with pytest.raises(ValueError):
        validate_qubit_sweep_configs(_cfgs(**over))


def test_input_widths_must_match():
    from quanonet_amd.qubit_sweep import validate_qubit_sweep_configs
    import numpy as np
    cs = _cfgs()
    datas = [{'train_branch_input': np.zeros((10, 4)), 'train_trunk_input': np.zeros((10, 1)), 'train_output': np.zeros((10, 1)),
              'test_branch_input': np.zeros((2, 4)), 'test_trunk_input': np.zeros((2, 1)), 'test_output': np.zeros((2, 1))}
             for _ in cs]
    datas[2] = dict(datas[2], train_branch_input=np.zeros((10, 5)))
    with pytest.raises(ValueError):
        validate_qubit_sweep_configs(cs, datas)


def test_ham_diag_per_member_length():
    from quanonet_amd.qubit_sweep import validate_qubit_sweep_configs
    cs = [dict(c, ham_diag=list(range(1 << c['num_qubits']))) for c in _cfgs()]
    assert validate_qubit_sweep_configs(cs) == cs
    cs[1] = dict(cs[1], ham_diag=[0.0] * 4)
    with pytest.raises(ValueError):
        validate_qubit_sweep_configs(cs)


def test_depth_sweep_still_rejects_differing_qubit_counts():
    from quanonet_amd.depth_sweep import validate_depth_sweep_configs
    with pytest.raises(ValueError):
        validate_depth_sweep_configs(_cfgs())


@pytest.mark.parametrize('over', [dict(world_size=2), dict(optimizer='sgd'), dict(num_qubits=1)])
def test_qubit_sweep_solver_rejects_before_touching_a_device(over):
    import torch
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    with pytest.raises(ValueError):
        QubitSweepSolver(_cfgs(**over), {}, device=torch.device('cpu'))
