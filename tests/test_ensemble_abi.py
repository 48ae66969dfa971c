"""
Model ensemble (qhea_model_ensemble_train_steps, quanonet_amd.ensemble): what can be checked without a GPU -- the exported
symbols, the workspace size, the argument checks that return before anything is launched, and EnsembleSolver's config
validation (done before any device is touched).
"""
import ctypes

import pytest

from quanonet_amd import _lib

QHEA_EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _desc():
    return _lib.make_model_desc(_lib.MODEL_QUANONET, 5, (40, 2, 20, 2), 100, 2, True, 0.1, 0.0, 1.0)


def test_ensemble_symbols_are_exported(lib):
    for name in ('qhea_model_ensemble_workspace_bytes', 'qhea_model_ensemble_train_steps'):
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert lib.qhea_version() >= 450


def test_ensemble_workspace_covers_every_member_and_grows_with_r(lib):
    d = _desc()
    single = lib.qhea_model_workspace_bytes(ctypes.byref(d), 100)
    assert single > 0
    prev = 0
    for r in (1, 2, 3, 5, 8, 15, 40):
        b = _lib.model_ensemble_workspace_bytes(d, r, 100)
        assert b >= r * single, r
        assert b >= prev, r
        prev = b
    assert _lib.model_ensemble_workspace_bytes(d, 0, 100) == 0


def _call(lib, d, n_models=3, grad_stride=None, branch=1, y=1, params=1, n_steps=2):
    P = _lib.model_param_count(d)
    rb = (ctypes.c_int64 * 3)(0, 100, 150)
    ib = (ctypes.c_double * 2)(0.01, 0.02)
    fake = ctypes.c_void_p(4096)                # never dereferenced: every case fails its checks first
    ptr = lambda v: fake if v else None
    return lib.qhea_model_ensemble_train_steps(ctypes.byref(d), n_models, n_steps, rb, ptr(branch), fake, ptr(y), ptr(params),
                                               None, ib, fake, P + 2 if grad_stride is None else grad_stride, fake, fake, 1,
                                               1e-3, 0.9, 0.999, 1e-8, 0.0, fake, 1 << 30, None)


def test_ensemble_rejects_bad_arguments_before_launching(lib):
    d = _desc()
    P = _lib.model_param_count(d)
    assert _call(lib, d, n_models=0) == QHEA_EINVAL
    assert _call(lib, d, n_models=-2) == QHEA_EINVAL
    assert _call(lib, d, n_steps=0) == QHEA_EINVAL
    assert _call(lib, d, grad_stride=P + 1) == QHEA_EINVAL
    assert _call(lib, d, branch=0) == QHEA_EINVAL
    assert _call(lib, d, y=0) == QHEA_EINVAL
    assert _call(lib, d, params=0) == QHEA_EINVAL


BASE = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'net_size': [5, 1, 5, 1], 'scale_coeff': 0.001,
        'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': 100, 'num_epochs': 2, 'prefix': 'out'}


def _cfgs(**over):
    cs = [dict(BASE, seed=s, run_id=f'seed{s}') for s in range(3)]
    cs[2].update(over)
    return cs


def test_ensemble_configs_may_differ_in_seed_run_and_prefix():
    from quanonet_amd.ensemble import validate_configs
    cs = _cfgs(prefix='elsewhere', scale_coeff=0.01)          # trainable frequency: scale_coeff is per member
    assert validate_configs(cs) == cs


@pytest.mark.parametrize('over', [dict(learning_rate=1e-3), dict(num_qubits=3), dict(batch_size=50), dict(net_size=[5, 1, 5, 2]),
                                  dict(num_epochs=3), dict(lr_scheduler='cosine'), dict(ham_pauli='X'),
                                  dict(if_trainable_freq='false')])
def test_ensemble_rejects_configs_that_differ_elsewhere(over):
    from quanonet_amd.ensemble import validate_configs
    with pytest.raises(ValueError):
        validate_configs(_cfgs(**over))


def test_ensemble_rejects_scale_difference_without_trainable_frequency():
    from quanonet_amd.ensemble import validate_configs
    cs = [dict(BASE, if_trainable_freq='false', seed=s) for s in range(2)]
    cs[1]['scale_coeff'] = 0.01
    with pytest.raises(ValueError):
        validate_configs(cs)


@pytest.mark.parametrize('over', [dict(world_size=2), dict(dp_exchange='peer'), dict(dp_calibrate=False), dict(optimizer='sgd'),
                                  dict(optimizer_kwargs={'amsgrad': True}), dict(epoch_call=False), dict(skip_completed=True)])
def test_ensemble_rejects_unsupported_settings_before_touching_a_device(over):
    import torch
    from quanonet_amd.ensemble import EnsembleSolver
    cs = [dict(BASE, seed=s, **over) for s in range(2)]
    with pytest.raises(ValueError):
        EnsembleSolver(cs, {}, device=torch.device('cpu'))
