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
from .depth_sweep import DEPTH_SWEEP_KEYS, DepthSweepSolver, validate_depth_sweep_configs
from .ensemble import check_shared, check_supported
from .sweep import SweepSolver, sweep_data

# keys in which the members of one qubit sweep may differ (net_size only in its depth entries)
QUBIT_SWEEP_KEYS = DEPTH_SWEEP_KEYS + ('num_qubits',)


def validate_qubit_sweep_configs(configs, data_dicts=None):
    """Raise ValueError unless `configs` (and `data_dicts`, when given) can train as one qubit sweep.  Touches no device."""
    configs = check_supported(configs, who='QubitSweepSolver')
    check_shared(configs, QUBIT_SWEEP_KEYS, what='one qubit sweep')
    for i, c in enumerate(configs):
        if 'num_qubits' not in c:
            raise ValueError(f"config {i} gives no num_qubits")
        n = int(c['num_qubits'])
        if n < 2:
            raise ValueError(f"config {i}'s num_qubits = {n}: a qubit sweep member needs at least 2 qubits")
        diag = c.get('ham_diag')
        if diag is not None and len(list(diag)) != 1 << n:
            raise ValueError(f"config {i}'s ham_diag has {len(list(diag))} entries, its {n} qubits need {1 << n}")
    # everything else is DepthSweepSolver's rule set, checked on the configs with num_qubits and ham_diag made equal
    n0 = int(configs[0]['num_qubits'])
    flat = [dict(c, num_qubits=n0) for c in configs]
    for c in flat:
        if c.get('ham_diag') is not None:
            c['ham_diag'] = [0.0] * (1 << n0)
    validate_depth_sweep_configs(flat, data_dicts)
    return configs


class QubitSweepSolver(DepthSweepSolver):
    """R PTSolver runs that differ in qubit count and circuit depth (and anything SweepSolver allows), trained together."""

    def __init__(self, configs, data_dicts, device=None, log=print):
        import torch
        self.configs = validate_qubit_sweep_configs(configs, data_dicts)
        SweepSolver._build(self, sweep_data(self.configs, data_dicts), device, log)
        self.descs = [m.trainer.desc for m in self.members]
        if any(d is None for d in self.descs):
            raise RuntimeError("QubitSweepSolver needs the fused model-level training path (QuanONetPT / HEAQNNPT in fp64)")
        diags = [m.trainer._ham_diag() for m in self.members]
        self.ham_diag = None
        if diags[0] is not None:            # [R, 2^nmax]: member m's spectrum at the front of row m
            width = max(d.numel() for d in diags)
            self.ham_diag = torch.zeros(len(diags), width, dtype=torch.float64, device=self.device)
            for i, d in enumerate(diags):
                self.ham_diag[i, :d.numel()].copy_(d.reshape(-1))

    def _train_steps(self, bounds, gbs, inputs, out, rows, first_step):
        """one epoch's steps of every member with its own qubit count, depth, read-out, scale and CURRENT learning rate"""
        from . import _lib
        hps = []
        for m, d in zip(self.members, self.descs):
            lr = m.trainer.optimizer.param_groups[0]['lr']
            hps.append(_lib.member_hparams(d.scale_coeff, d.ham_offset, d.ham_coeff, lr, d.ham_pauli))
        g = self.members[0].trainer.optimizer.param_groups[0]
        _lib.model_qubit_sweep_train_steps(self.descs, hps, bounds, gbs, inputs[0], inputs[1] if len(inputs) > 1 else None, out,
                                           self.params, rows, self.exp_avg, self.exp_avg_sq, first_step, g['betas'][0],
                                           g['betas'][1], g['eps'], g['weight_decay'], ham_diag=self.ham_diag)
