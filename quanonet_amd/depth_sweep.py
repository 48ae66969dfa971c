"""
Depth sweeps as one ensemble: the cells of a capacity grid -- circuits of different branch / trunk depths -- trained side by side
on one device, every step of all R members as one launch per kernel (qhea_model_depth_sweep_train_steps).  The reference runs
such grids (scripts/reproduce_capacity.sh, reproduce_circuit.sh, reproduce_scaling.sh: net_size = hb 2 ht 2 over hb x ht x
seeds) as one training process per cell and seed.

Members may differ in everything SweepSolver allows (seed, run_id, prefix, read-out, frequency scale, learning rate and its
schedule, operator) and in the depth entries of net_size: QuanONet net_size[0] (branch depth) and net_size[2] (trunk depth),
HEAQNN net_size[0].  The qubit count, the linear depths, the input widths, the model type and the frequency mode are shared.
Member m is exactly the PTSolver run its config describes when launched after ``set_random_seed(seed_m)``, with its own
checkpoints and history.  The parameters of all members live in one [R, Pmax] device tensor (Pmax = the largest member's
parameter count); member m's model parameters are views into the front of row m.
"""
from .ensemble import check_shared, check_supported
from .solver import model_setting
from .sweep import SWEEP_KEYS, SweepSolver, check_sweep_rules

# keys in which the members of one depth sweep may differ (net_size only in its depth entries: _check_net_sizes)
DEPTH_SWEEP_KEYS = SWEEP_KEYS + ('net_size',)


def _depth_entries(cfg):
    """indices of net_size that are depths for the config's model type"""
    return (0, 2) if str(cfg.get('model_type', 'QuanONet')).lower() == 'quanonet' else (0,)


def _check_net_sizes(configs):
    ref = list(model_setting(configs[0], 'net_size'))
    free = _depth_entries(configs[0])
    for i, c in enumerate(configs):
        net = list(model_setting(c, 'net_size'))
        if len(net) != len(ref):
            raise ValueError(f"config {i}'s net_size {net} has a different length than config 0's {ref}")
        for k, (a, b) in enumerate(zip(ref, net)):
            if k not in free and a != b:
                raise ValueError(f"config {i}'s net_size {net} differs from config 0's {ref} in entry {k}: members of one "
                                 f"depth sweep may differ only in the depth entries {list(free)}")
        for k in free:
            if int(net[k]) < 0:
                raise ValueError(f"config {i}'s net_size {net} has a negative depth")


def validate_depth_sweep_configs(configs, data_dicts=None):
    """Raise ValueError unless `configs` (and `data_dicts`, when given) can train as one depth sweep.  Touches no device."""
    configs = check_supported(configs, who='DepthSweepSolver')
    check_shared(configs, DEPTH_SWEEP_KEYS, what='one depth sweep')
    _check_net_sizes(configs)
    check_sweep_rules(configs, data_dicts)
    return configs


class DepthSweepSolver(SweepSolver):
    """R PTSolver runs that differ in circuit depth (and anything SweepSolver allows), trained together."""
    validate = staticmethod(validate_depth_sweep_configs)
    entry = 'model_depth_sweep_train_steps'
    takes_descs = True
