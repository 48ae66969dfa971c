"""
Ablation sweeps as one ensemble: the cells of a hyper-parameter grid of ONE circuit shape trained side by side on one device,
every step of all R members as one launch per kernel (qhea_model_sweep_train_steps).  The reference runs such grids
(scripts/reproduce_hamiltonian.sh: --ham_pauli, --ham_bound, --ham_diag x seeds; scripts/reproduce_benchmarks1.sh:
--scale_coeff x seeds, operators that share input widths) as one training process per cell and seed.

Members may differ in what EnsembleSolver allows (seed, run_id, prefix) and in the read-out (ham_bound, ham_pauli, ham_diag),
the frequency scale (scale_coeff, fixed or trainable frequency), the learning rate and its schedule (learning_rate,
lr_scheduler, lr_scheduler_kwargs) and the training data (operator, with one data dict per member).  Member m is exactly the
PTSolver run its config describes when launched after ``set_random_seed(seed_m)``, on its own data dict, with its own
checkpoints -- as in quanonet_amd.ensemble, whose solver this one is a kind of.
"""
import os

from .ensemble import MEMBER_KEYS, PerMemberSolver, check_shared, check_supported
from .ensemble import sweep_data            # (the member solver's __init__ needs it there; its public name is this module's)
from .solver import run_dir

# keys in which the members of one sweep may differ
SWEEP_KEYS = MEMBER_KEYS + ('ham_bound', 'ham_pauli', 'ham_diag', 'scale_coeff', 'learning_rate', 'lr_scheduler',
                            'lr_scheduler_kwargs', 'operator')


def check_sweep_rules(configs, data_dicts):
    """What a sweep of any kind asks beyond its shared keys: a ham_diag for every member or for none, a directory of its own
    for every member, train arrays of one shape (`data_dicts` None: not checked)."""
    has_diag = [c.get('ham_diag') is not None for c in configs]
    if any(has_diag) and not all(has_diag):
        raise ValueError("either every member of a sweep reads out a ham_diag or none does")
    seen = {}
    for i, c in enumerate(configs):
        d = os.path.normpath(run_dir(c))
        if d in seen:
            raise ValueError(f"configs {seen[d]} and {i} would both write to {d!r}: give them distinct run_id / prefix")
        seen[d] = i
    if data_dicts is not None:
        sweep_data(configs, data_dicts)


def validate_sweep_configs(configs, data_dicts=None):
    """Raise ValueError unless `configs` (and `data_dicts`, when given) can train as one sweep.  Touches no device."""
    configs = check_supported(configs, who='SweepSolver')
    check_shared(configs, SWEEP_KEYS, what='one sweep')
    check_sweep_rules(configs, data_dicts)
    return configs


class SweepSolver(PerMemberSolver):
    """R PTSolver runs of one circuit shape that differ in read-out, scale, learning rate or data, trained together."""
    validate = staticmethod(validate_sweep_configs)
    entry = 'model_sweep_train_steps'
