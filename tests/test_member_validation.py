"""
What the four member validators refuse and accept (quanonet_amd.ensemble / sweep / depth_sweep / qubit_sweep: validate_configs,
validate_sweep_configs, validate_depth_sweep_configs, validate_qubit_sweep_configs).  Pure Python: no library, no device.

Every rule of every level has at least one rejected input here, with the exception's exact text.  The texts were recorded by
running the validators of commit 19486c5 (the last one in which each level re-validated flattened copies of its configs through
the level below) on these very inputs: a level that calls the rule sets below it directly must refuse the same inputs with the
same words, and where an input breaks two rules, with the words of the same one.
"""
import numpy as np
import pytest

BASE = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'net_size': [5, 1, 5, 1], 'scale_coeff': 0.001,
        'if_trainable_freq': 'true', 'learning_rate': 1e-3, 'batch_size': 100, 'num_epochs': 2}
HEA = dict(BASE, model_type='HEAQNN', net_size=[3, 2])


def _members(n=2, base=BASE, **common):
    return [dict(base, seed=s, run_id=f's{s}', **common) for s in range(n)]


def _with(i, cfgs=None, drop=(), **changes):
    """the members with config i changed (and keys of `drop` removed from it)"""
    cfgs = _members() if cfgs is None else cfgs
    cfgs[i] = {k: v for k, v in dict(cfgs[i], **changes).items() if k not in drop}
    return cfgs


def _data(rows=10, width=3, **extra):
    return dict({'train_branch_input': np.zeros((rows, width)), 'train_trunk_input': np.zeros((rows, 1)),
                 'train_output': np.zeros((rows, 1)), 'test_output': np.zeros((4, 1))}, **extra)


def _validator(name):
    from quanonet_amd import depth_sweep, ensemble, qubit_sweep, sweep
    return {'ensemble': ensemble.validate_configs, 'sweep': sweep.validate_sweep_configs,
            'depth': depth_sweep.validate_depth_sweep_configs, 'qubit': qubit_sweep.validate_qubit_sweep_configs}[name]


LEVELS = ('ensemble', 'sweep', 'depth', 'qubit')
WHO = {'ensemble': 'EnsembleSolver', 'sweep': 'SweepSolver', 'depth': 'DepthSweepSolver', 'qubit': 'QubitSweepSolver'}

# ---- unsupported settings: check_supported, once per level and under the level's own name -------------------------------------
UNSUPPORTED = {
    'no_configs': (lambda: [], "{who} needs at least one config"),
    'world_size': (lambda: _with(1, world_size=2), "{who} runs on one device: world_size > 1 is not supported"),
    'dp_keys': (lambda: _with(0, dp_exchange='rccl', dp_calibrate=False),
                "{who} has no data-parallel step: remove ['dp_calibrate', 'dp_exchange']"),
    'optimizer': (lambda: _with(1, optimizer='sgd'), "{who} trains with Adam only (got optimizer='sgd')"),
    'optimizer_kwargs': (lambda: _with(0, optimizer_kwargs={'amsgrad': True, 'eps': 1e-9}),
                         "{who}'s Adam takes betas / eps / weight_decay only (got ['amsgrad'])"),
    'epoch_call': (lambda: _with(1, epoch_call=False),
                   "{who} issues each epoch from one host call: epoch_call=False is not supported"),
    'skip_completed': (lambda: _with(0, skip_completed=True), "{who} trains every member: skip_completed is not supported"),
}

_FREE = {
    'ensemble': "['prefix', 'run_id', 'scale_coeff', 'seed']",
    'sweep': "['ham_bound', 'ham_diag', 'ham_pauli', 'learning_rate', 'lr_scheduler', 'lr_scheduler_kwargs', 'operator', "
             "'prefix', 'run_id', 'scale_coeff', 'seed']",
    'depth': "['ham_bound', 'ham_diag', 'ham_pauli', 'learning_rate', 'lr_scheduler', 'lr_scheduler_kwargs', 'net_size', "
             "'operator', 'prefix', 'run_id', 'scale_coeff', 'seed']",
    'qubit': "['ham_bound', 'ham_diag', 'ham_pauli', 'learning_rate', 'lr_scheduler', 'lr_scheduler_kwargs', 'net_size', "
             "'num_qubits', 'operator', 'prefix', 'run_id', 'scale_coeff', 'seed']",
}
_SWEEPS = ('sweep', 'depth', 'qubit')
_DEPTHS = ('depth', 'qubit')
_D4 = [0.0, 1.0, 2.0, 3.0]

# (levels, case, configs, data dicts or None, message): the message is the parent commit's, verbatim
REJECTED = [
    # ---- a differing key outside the level's free keys: check_shared, once per level ------------------------------------------
    (('ensemble',), 'differs_lr', lambda: _with(1, learning_rate=2e-3), None,
     "config 1 differs from config 0 in 'learning_rate' (0.002 vs 0.001): members of one ensemble may differ only in "
     + _FREE['ensemble']),
    (('ensemble',), 'differs_fixed_scale', lambda: _with(1, _members(if_trainable_freq='false'), scale_coeff=0.1), None,
     "config 1 differs from config 0 in 'scale_coeff' (0.1 vs 0.001): members of one ensemble may differ only in "
     "['prefix', 'run_id', 'seed']"),
    (('ensemble',), 'differs_key_absent', lambda: _with(2, _members(3), ham_pauli='X'), None,
     "config 2 differs from config 0 in 'ham_pauli' ('X' vs None): members of one ensemble may differ only in "
     + _FREE['ensemble']),
    (('sweep',), 'differs_net_size', lambda: _with(1, net_size=[6, 1, 5, 1]), None,
     "config 1 differs from config 0 in 'net_size' ([6, 1, 5, 1] vs [5, 1, 5, 1]): members of one sweep may differ only in "
     + _FREE['sweep']),
    (('sweep', 'depth'), 'differs_num_qubits', lambda: _with(1, num_qubits=3), None,
     "config 1 differs from config 0 in 'num_qubits' (3 vs 2): members of {what} may differ only in {free}"),
    (_SWEEPS, 'differs_batch_size', lambda: _with(1, batch_size=50), None,
     "config 1 differs from config 0 in 'batch_size' (50 vs 100): members of {what} may differ only in {free}"),
    (_SWEEPS, 'differs_model_type', lambda: _with(1, model_type='HEAQNN'), None,
     "config 1 differs from config 0 in 'model_type' ('HEAQNN' vs 'QuanONet'): members of {what} may differ only in {free}"),
    # ---- SweepSolver's rule set, at every level above it on the real configs --------------------------------------------------
    (_SWEEPS, 'mixed_ham_diag', lambda: _with(1, ham_diag=_D4), None,
     "either every member of a sweep reads out a ham_diag or none does"),
    (_SWEEPS, 'mixed_ham_diag_first', lambda: _with(0, _members(3), ham_diag=_D4), None,
     "either every member of a sweep reads out a ham_diag or none does"),
    (_SWEEPS, 'duplicate_dir', lambda: _with(1, run_id='s0'), None,
     "configs 0 and 1 would both write to 'outputs/Antideriv/s0': give them distinct run_id / prefix"),
    (_SWEEPS, 'duplicate_dir_normpath', lambda: _with(2, _members(3, prefix='out/x'), prefix='out/./x/', run_id='s1'), None,
     "configs 1 and 2 would both write to 'out/x/Antideriv/s1': give them distinct run_id / prefix"),
    (_SWEEPS, 'duplicate_dir_defaults', lambda: [{k: v for k, v in c.items() if k not in ('run_id', 'operator')}
                                                 for c in _members()], None,
     "configs 0 and 1 would both write to 'outputs/Op/run': give them distinct run_id / prefix"),
    (_SWEEPS, 'data_count', _members, lambda: [_data(), _data(), _data()],
     "3 data dicts for 2 configs: give one dict, or one per config"),
    (_SWEEPS, 'data_shape', _members, lambda: [_data(), _data(rows=11)],
     "data dict 1's 'train_branch_input' has shape (11, 3), data dict 0's (10, 3): every member trains on arrays of one shape"),
    (_SWEEPS, 'data_width', lambda: _members(3), lambda: [_data(), _data(), _data(width=4)],
     "data dict 2's 'train_branch_input' has shape (10, 4), data dict 0's (10, 3): every member trains on arrays of one shape"),
    (_SWEEPS, 'data_key_missing', _members, lambda: [_data(), {k: v for k, v in _data().items() if k != 'train_output'}],
     "data dict 1's 'train_output' has shape (), data dict 0's (10, 1): every member trains on arrays of one shape"),
    # ---- DepthSweepSolver's net_size rules, also under QubitSweepSolver --------------------------------------------------------
    (_DEPTHS, 'net_linear_depth', lambda: _with(1, net_size=[7, 2, 5, 1]), None,
     "config 1's net_size [7, 2, 5, 1] differs from config 0's [5, 1, 5, 1] in entry 1: members of one depth sweep may differ "
     "only in the depth entries [0, 2]"),
    (_DEPTHS, 'net_last_entry', lambda: _with(2, _members(3), net_size=[5, 1, 9, 2]), None,
     "config 2's net_size [5, 1, 9, 2] differs from config 0's [5, 1, 5, 1] in entry 3: members of one depth sweep may differ "
     "only in the depth entries [0, 2]"),
    (_DEPTHS, 'net_against_default', lambda: _with(0, _with(1, net_size=[20, 2, 10, 3]), drop=('net_size',)), None,
     "config 1's net_size [20, 2, 10, 3] differs from config 0's [20, 2, 10, 2] in entry 3: members of one depth sweep may "
     "differ only in the depth entries [0, 2]"),
    (_DEPTHS, 'net_heaqnn_linear_depth', lambda: _with(1, _members(base=HEA), net_size=[4, 3]), None,
     "config 1's net_size [4, 3] differs from config 0's [3, 2] in entry 1: members of one depth sweep may differ only in the "
     "depth entries [0]"),
    (_DEPTHS, 'net_length', lambda: _with(1, net_size=[5, 1]), None,
     "config 1's net_size [5, 1] has a different length than config 0's [5, 1, 5, 1]"),
    (_DEPTHS, 'net_negative_depth', lambda: _with(1, net_size=[5, 1, -1, 1]), None,
     "config 1's net_size [5, 1, -1, 1] has a negative depth"),
    (_DEPTHS, 'net_negative_depth_first', lambda: _with(0, net_size=[-2, 1, 5, 1]), None,
     "config 0's net_size [-2, 1, 5, 1] has a negative depth"),
    # ---- QubitSweepSolver's own rules ------------------------------------------------------------------------------------------
    (('qubit',), 'no_num_qubits', lambda: _with(1, drop=('num_qubits',)), None, "config 1 gives no num_qubits"),
    (('qubit',), 'no_num_qubits_anywhere', lambda: [{k: v for k, v in c.items() if k != 'num_qubits'} for c in _members()],
     None, "config 0 gives no num_qubits"),
    (('qubit',), 'one_qubit', lambda: _with(1, num_qubits=1), None,
     "config 1's num_qubits = 1: a qubit sweep member needs at least 2 qubits"),
    (('qubit',), 'ham_diag_length', lambda: _with(1, _members(ham_diag=_D4), num_qubits=3), None,
     "config 1's ham_diag has 4 entries, its 3 qubits need 8"),
    (('qubit',), 'ham_diag_length_first', lambda: _members(ham_diag=_D4 + [4.0]), None,
     "config 0's ham_diag has 5 entries, its 2 qubits need 4"),
    # ---- inputs that break two rules: the words are those of the rule the parent reached first ---------------------------------
    (_DEPTHS, 'net_before_duplicate_dir', lambda: _with(1, net_size=[5, 2, 5, 1], run_id='s0'), None,
     "config 1's net_size [5, 2, 5, 1] differs from config 0's [5, 1, 5, 1] in entry 1: members of one depth sweep may differ "
     "only in the depth entries [0, 2]"),
    (_DEPTHS, 'net_before_mixed_ham_diag', lambda: _with(1, net_size=[5, 1], ham_diag=_D4), None,
     "config 1's net_size [5, 1] has a different length than config 0's [5, 1, 5, 1]"),
    (('qubit',), 'qubits_before_net', lambda: _with(1, num_qubits=0, net_size=[5, 2, 5, 1]), None,
     "config 1's num_qubits = 0: a qubit sweep member needs at least 2 qubits"),
    (('qubit',), 'ham_diag_length_before_mixed', lambda: _with(1, num_qubits=3, ham_diag=_D4), None,
     "config 1's ham_diag has 4 entries, its 3 qubits need 8"),
    (_SWEEPS, 'mixed_ham_diag_before_duplicate_dir', lambda: _with(1, ham_diag=_D4, run_id='s0'), None,
     "either every member of a sweep reads out a ham_diag or none does"),
    (_SWEEPS, 'duplicate_dir_before_data', lambda: _with(1, run_id='s0'), lambda: [_data()],
     "configs 0 and 1 would both write to 'outputs/Antideriv/s0': give them distinct run_id / prefix"),
    (_SWEEPS, 'shared_before_data', lambda: _with(1, num_epochs=3), lambda: [_data()],
     "config 1 differs from config 0 in 'num_epochs' (3 vs 2): members of {what} may differ only in {free}"),
]
WHAT = {'ensemble': 'one ensemble', 'sweep': 'one sweep', 'depth': 'one depth sweep', 'qubit': 'one qubit sweep'}


def _rejected_cases():
    for case, (make, msg) in UNSUPPORTED.items():
        for level in LEVELS:
            yield pytest.param(level, make, None, msg.format(who=WHO[level]), id=f'{level}-{case}')
    for levels, case, make, data, msg in REJECTED:
        for level in levels:
            yield pytest.param(level, make, data, msg.replace('{what}', WHAT[level]).replace('{free}', _FREE[level]),
                               id=f'{level}-{case}')


@pytest.mark.parametrize('level,make,data,message', list(_rejected_cases()))
def test_rejected_input_raises_the_recorded_message(level, make, data, message):
    args = (make(),) if data is None else (make(), data())
    with pytest.raises(ValueError) as e:
        _validator(level)(*args)
    assert type(e.value) is ValueError and str(e.value) == message


_SWEEP_FREE = dict(ham_bound=[-2, 2], ham_pauli='X', scale_coeff=0.1, learning_rate=5e-3, lr_scheduler='step',
                   lr_scheduler_kwargs={'step_size': 1}, operator='Other', prefix='elsewhere')
ACCEPTED = [
    (LEVELS, 'one_member', lambda: _members(1), None),
    (LEVELS, 'seeds', lambda: _members(3), None),
    (LEVELS, 'trainable_scales', lambda: _with(1, scale_coeff=0.1, prefix='p'), None),
    (LEVELS, 'adam_settings', lambda: _members(optimizer='Adam', optimizer_kwargs={'betas': (0.8, 0.9), 'eps': 1e-9},
                                               world_size=1, epoch_call=True, skip_completed=False), None),
    (_SWEEPS, 'sweep_keys', lambda: _with(1, **_SWEEP_FREE), None),
    (_SWEEPS, 'fixed_scales', lambda: _with(1, _members(if_trainable_freq='false'), scale_coeff=0.1), None),
    (_SWEEPS, 'every_member_a_ham_diag', lambda: _with(1, _members(ham_diag=_D4), ham_diag=[1.0, 0.0, 0.0, -1.0]), None),
    (_SWEEPS, 'same_run_id_other_operator', lambda: _with(1, run_id='s0', operator='Other'), None),
    (_SWEEPS, 'shared_data_dict', _members, _data),
    (_SWEEPS, 'data_per_member', _members, lambda: [_data(), _data(extra_test_rows=np.zeros(7))]),
    (_SWEEPS, 'test_sets_differ', _members, lambda: [_data(), _data(test_output=np.zeros((9, 1)))]),
    (_DEPTHS, 'depths', lambda: _with(1, net_size=[40, 1, 0, 1], **_SWEEP_FREE), None),
    (_DEPTHS, 'depths_against_default', lambda: _with(0, _with(1, net_size=[3, 2, 7, 2]), drop=('net_size',)), None),
    (_DEPTHS, 'heaqnn_depths', lambda: _with(1, _members(base=HEA), net_size=[9, 2]), _data),
    (('qubit',), 'qubits', lambda: _with(1, num_qubits=7, net_size=[1, 1, 2, 1]), None),
    (('qubit',), 'qubits_and_ham_diags', lambda: _with(1, _members(ham_diag=_D4), num_qubits=3, ham_diag=[0.5] * 8), _data),
]


@pytest.mark.parametrize('level,make,data', [pytest.param(level, make, data, id=f'{level}-{case}')
                                             for levels, case, make, data in ACCEPTED for level in levels])
def test_accepted_input_is_returned_unchanged(level, make, data):
    configs = make()
    args = (configs,) if data is None else (configs, data())
    got = _validator(level)(*args)
    assert got == make() and all(g is c for g, c in zip(got, configs))
