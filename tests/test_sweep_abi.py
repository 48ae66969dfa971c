"""
Model sweep (qhea_model_sweep_train_steps, quanonet_amd.sweep): what can be checked without a GPU -- the exported symbols and
the member-record struct, the workspace size, the argument checks that return before anything is launched, and SweepSolver's
config validation (done before any device is touched).
"""
import ctypes
import math

import pytest

from quanonet_amd import _lib

QHEA_EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _desc():
    return _lib.make_model_desc(_lib.MODEL_QUANONET, 5, (40, 2, 20, 2), 100, 2, True, 0.1, 0.0, 1.0)


def test_sweep_symbols_are_exported(lib):
    for name in ('qhea_model_sweep_workspace_bytes', 'qhea_model_sweep_train_steps'):
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert lib.qhea_version() >= 460


def test_member_record_matches_the_header():
    M = _lib.MemberHParams
    assert ctypes.sizeof(M) == 40
    assert [(n, getattr(M, n).offset) for n, _ in M._fields_] == [
        ('scale_coeff', 0), ('ham_offset', 8), ('ham_coeff', 16), ('lr', 24), ('ham_pauli', 32), ('reserved', 36)]


@pytest.mark.parametrize('R', [1, 5, 50])
def test_sweep_workspace_covers_the_ensemble_one(lib, R):
    d = _desc()
    assert _lib.model_sweep_workspace_bytes(d, R, 100) >= _lib.model_ensemble_workspace_bytes(d, R, 100) > 0


def _call(lib, d, members, n_models=None, diag=False):
    P = _lib.model_param_count(d)
    R = len(members) if n_models is None else n_models
    rb = (ctypes.c_int64 * 3)(0, 100, 150)
    ib = (ctypes.c_double * 2)(0.01, 0.02)
    fake = ctypes.c_void_p(4096)                # never dereferenced: every case fails its checks first
    mh = (_lib.MemberHParams * max(1, len(members)))(*members) if members is not None else None
    return lib.qhea_model_sweep_train_steps(ctypes.byref(d), R, mh, fake if diag else None, 2, rb, fake, fake, fake, fake, ib,
                                            fake, P + 2, fake, fake, 1, 0.9, 0.999, 1e-8, 0.0, fake, 1 << 30, None)


def _m(pauli=0, lr=1e-3):
    m = _lib.MemberHParams(0.1, 0.0, 1.0, 1e-3, 0, 0)
    m.ham_pauli, m.lr = pauli, lr
    return m


def test_sweep_rejects_bad_arguments_before_launching(lib):
    d = _desc()
    assert _call(lib, d, [_m()], n_models=0) == QHEA_EINVAL
    assert _call(lib, d, [_m()], n_models=-1) == QHEA_EINVAL
    assert _call(lib, d, None, n_models=2) == QHEA_EINVAL
    assert _call(lib, d, [_m(), _m(pauli=3)]) == QHEA_EINVAL
    assert _call(lib, d, [_m(), _m(pauli=-1)]) == QHEA_EINVAL
    assert _call(lib, d, [_m(), _m(pauli=1)], diag=True) == QHEA_EINVAL
    for lr in (-1e-3, math.nan, math.inf):
        assert _call(lib, d, [_m(), _m(lr=lr)]) == QHEA_EINVAL, lr


BASE = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'net_size': [5, 1, 5, 1], 'scale_coeff': 0.001,
        'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': 100, 'num_epochs': 2, 'prefix': 'out'}


def _cfgs(**over):
    cs = [dict(BASE, seed=s, run_id=f'seed{s}') for s in range(3)]
    cs[2].update(over)
    return cs


@pytest.mark.parametrize('over', [dict(ham_bound=[-2, 2]), dict(ham_pauli='X'), dict(scale_coeff=0.1),
                                  dict(learning_rate=1e-3), dict(lr_scheduler='step'),
                                  dict(lr_scheduler='step', lr_scheduler_kwargs={'step_size': 1}), dict(operator='Other'),
                                  dict(prefix='elsewhere')])
def test_sweep_configs_may_differ_in_the_new_keys(over):
    from quanonet_amd.sweep import validate_sweep_configs
    cs = _cfgs(**over)
    assert validate_sweep_configs(cs) == cs


def test_sweep_fixed_frequency_scales_and_diag_spectra_may_differ():
    from quanonet_amd.sweep import validate_sweep_configs
    cs = [dict(BASE, if_trainable_freq='false', seed=0, run_id=f'r{i}', scale_coeff=s) for i, s in enumerate((0.1, 0.01))]
    assert validate_sweep_configs(cs) == cs
    cs = [dict(BASE, seed=0, run_id=f'r{i}', ham_diag=h) for i, h in enumerate(([-5, 5, 5, 5], [-5, 0, 0, 5]))]
    assert validate_sweep_configs(cs) == cs


@pytest.mark.parametrize('over', [dict(num_qubits=3), dict(net_size=[5, 1, 5, 2]), dict(model_type='HEAQNN'),
                                  dict(if_trainable_freq='false'), dict(batch_size=50), dict(num_epochs=3),
                                  dict(optimizer_kwargs={'eps': 1e-6}), dict(ham_diag=[-5, 5, 5, 5]),
                                  dict(run_id='seed0')])
def test_sweep_rejects_configs_that_differ_elsewhere(over):
    from quanonet_amd.sweep import validate_sweep_configs
    with pytest.raises(ValueError):
        validate_sweep_configs(_cfgs(**over))


def test_sweep_rejects_other_optimizers():
    from quanonet_amd.sweep import validate_sweep_configs
    with pytest.raises(ValueError):
        validate_sweep_configs([dict(BASE, seed=s, run_id=f'seed{s}', optimizer='sgd') for s in range(2)])


def _data(rows=10, test=4):
    import numpy as np
    return {'train_branch_input': np.zeros((rows, 10)), 'train_trunk_input': np.zeros((rows, 1)),
            'train_output': np.zeros((rows, 1)), 'test_branch_input': np.zeros((test, 10)),
            'test_trunk_input': np.zeros((test, 1)), 'test_output': np.zeros((test, 1))}


def test_sweep_data_lists():
    from quanonet_amd.sweep import validate_sweep_configs
    cs = _cfgs(operator='Other')
    assert validate_sweep_configs(cs, _data()) == cs
    assert validate_sweep_configs(cs, [_data(), _data(test=7), _data()]) == cs          # test sets may differ
    with pytest.raises(ValueError):
        validate_sweep_configs(cs, [_data(), _data()])
    with pytest.raises(ValueError):
        validate_sweep_configs(cs, [_data(), _data(rows=11), _data()])


@pytest.mark.parametrize('over', [dict(world_size=2), dict(dp_exchange='peer'), dict(epoch_call=False), dict(skip_completed=True)])
def test_sweep_solver_rejects_unsupported_settings_before_touching_a_device(over):
    import torch
    from quanonet_amd.sweep import SweepSolver
    cs = [dict(BASE, seed=s, run_id=f'seed{s}', **over) for s in range(2)]
    with pytest.raises(ValueError):
        SweepSolver(cs, {}, device=torch.device('cpu'))
