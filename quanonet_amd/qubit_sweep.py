"""
Qubit sweeps as one ensemble: the cells of a scaling grid -- circuits of different qubit counts and depths -- trained side by side
on one device (qhea_model_qubit_sweep_train_steps).  The reference runs such grids (scripts/reproduce_scaling.sh: Q2..Q8 with
P = 2^n, each with its own hb x ht list, x seeds; scripts/reproduce_circuit.sh: Q2, Q5, Q10) as one training process per cell
and seed; DepthSweepSolver takes one qubit count at a time.

Members may differ in everything DepthSweepSolver allows and in num_qubits (>= 2).  The linear depths, the input widths, the
model type and the frequency mode are shared; a member's ham_diag has 2^num_qubits entries.  Every step of all members is one
prep launch, one backward launch per register class (n <= 6) or qubit count (n = 7..12) present and one reduce launch.
Member m is exactly the PTSolver run its config describes when launched after
``set_random_seed(seed_m)``, with its own checkpoints and history.  The parameters of all members live in one [R, Pmax] device
tensor; member m's model parameters are views into the front of row m.
"""
from .depth_sweep import DEPTH_SWEEP_KEYS, DepthSweepSolver, _check_net_sizes
from .ensemble import check_shared, check_supported
from .sweep import check_sweep_rules

# keys in which the members of one qubit sweep may differ (net_size only in its depth entries)
QUBIT_SWEEP_KEYS = DEPTH_SWEEP_KEYS + ('num_qubits',)


def _check_qubits(configs):
    for i, c in enumerate(configs):
        if 'num_qubits' not in c:
            raise ValueError(f"config {i} gives no num_qubits")
        n = int(c['num_qubits'])
        if n < 2:
            raise ValueError(f"config {i}'s num_qubits = {n}: a qubit sweep member needs at least 2 qubits")
        diag = c.get('ham_diag')
        if diag is not None and len(list(diag)) != 1 << n:
            raise ValueError(f"config {i}'s ham_diag has {len(list(diag))} entries, its {n} qubits need {1 << n}")


def validate_qubit_sweep_configs(configs, data_dicts=None):
    """Raise ValueError unless `configs` (and `data_dicts`, when given) can train as one qubit sweep.  Touches no device."""
    configs = check_supported(configs, who='QubitSweepSolver')
    check_shared(configs, QUBIT_SWEEP_KEYS, what='one qubit sweep')
    _check_qubits(configs)
    _check_net_sizes(configs)
    check_sweep_rules(configs, data_dicts)
    return configs


class QubitSweepSolver(DepthSweepSolver):
    """R PTSolver runs that differ in qubit count and circuit depth (and anything SweepSolver allows), trained together."""
    validate = staticmethod(validate_qubit_sweep_configs)
    entry = 'model_qubit_sweep_train_steps'
