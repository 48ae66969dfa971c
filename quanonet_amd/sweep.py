"""
Ablation sweeps as one ensemble: the cells of a hyper-parameter grid of ONE circuit shape trained side by side on one device,
every step of all R members as one launch per kernel (qhea_model_sweep_train_steps).  The reference runs such grids
(scripts/reproduce_hamiltonian.sh: --ham_pauli, --ham_bound, --ham_diag x seeds; scripts/reproduce_benchmarks1.sh:
--scale_coeff x seeds, operators that share input widths) as one training process per cell and seed.

Members may differ in what EnsembleSolver allows (seed, run_id, prefix) and in the read-out (ham_bound, ham_pauli, ham_diag),
the frequency scale (scale_coeff, fixed or trainable frequency), the learning rate and its schedule (learning_rate,
lr_scheduler, lr_scheduler_kwargs) and the training data (operator, with one data dict per member).  Member m is exactly the
PTSolver run its config describes when launched after ``set_random_seed(seed_m)``, on its own data dict, with its own
checkpoints -- as in quanonet_amd.ensemble, whose solver this one extends.
"""
import os

import numpy as np

from .ensemble import MEMBER_KEYS, EnsembleSolver, check_shared, check_supported

# keys in which the members of one sweep may differ
SWEEP_KEYS = MEMBER_KEYS + ('ham_bound', 'ham_pauli', 'ham_diag', 'scale_coeff', 'learning_rate', 'lr_scheduler',
                            'lr_scheduler_kwargs', 'operator')


def _out_dir(c):
    """the directory PTSolver(c) writes to"""
    return os.path.normpath(os.path.join(c.get('prefix') or 'outputs', c.get('operator', 'Op'), c.get('run_id', 'run')))


def sweep_data(configs, data_dicts):
    """One data dict per member: `data_dicts` is one dict (shared) or a list of len(configs).  Every member's train arrays
    must have the same shapes (one schedule for all); test sets may differ."""
    if isinstance(data_dicts, dict):
        return [data_dicts] * len(configs)
    datas = list(data_dicts)
    if len(datas) != len(configs):
        raise ValueError(f"{len(datas)} data dicts for {len(configs)} configs: give one dict, or one per config")
    ref = datas[0]
    for i, d in enumerate(datas[1:], 1):
        keys = sorted(k for k in set(ref) | set(d) if k.startswith('train_'))
        for k in keys:
            if k not in ref or k not in d or np.shape(ref[k]) != np.shape(d[k]):
                raise ValueError(f"data dict {i}'s {k!r} has shape {np.shape(d.get(k))}, data dict 0's "
                                 f"{np.shape(ref.get(k))}: every member trains on arrays of one shape")
    return datas


def validate_sweep_configs(configs, data_dicts=None):
    """Raise ValueError unless `configs` (and `data_dicts`, when given) can train as one sweep.  Touches no device."""
    configs = check_supported(configs, who='SweepSolver')
    check_shared(configs, SWEEP_KEYS, what='one sweep')
    has_diag = [c.get('ham_diag') is not None for c in configs]
    if any(has_diag) and not all(has_diag):
        raise ValueError("either every member of a sweep reads out a ham_diag or none does")
    seen = {}
    for i, c in enumerate(configs):
        d = _out_dir(c)
        if d in seen:
            raise ValueError(f"configs {seen[d]} and {i} would both write to {d!r}: give them distinct run_id / prefix")
        seen[d] = i
    if data_dicts is not None:
        sweep_data(configs, data_dicts)
    return configs


class SweepSolver(EnsembleSolver):
    """R PTSolver runs of one circuit shape that differ in read-out, scale, learning rate or data, trained together."""

    def __init__(self, configs, data_dicts, device=None, log=print):
        self.configs = validate_sweep_configs(configs, data_dicts)
        self._build(sweep_data(self.configs, data_dicts), device, log)
        self.descs = [m.trainer.desc for m in self.members]
        if any(d is None for d in self.descs):
            raise RuntimeError("SweepSolver needs the fused model-level training path (QuanONetPT / HEAQNNPT in fp64)")
        diags = [m.trainer._ham_diag() for m in self.members]
        self.ham_diag = None
        if diags[0] is not None:
            import torch
            self.ham_diag = torch.stack([d.reshape(-1) for d in diags]).to(self.device, dtype=torch.float64).contiguous()

    def _train_steps(self, bounds, gbs, inputs, out, rows, first_step):
        """one epoch's steps of every member with its own read-out, scale and CURRENT learning rate (its scheduler has
        stepped), one launch per kernel and step"""
        from . import _lib
        hps = []
        for m, d in zip(self.members, self.descs):
            lr = m.trainer.optimizer.param_groups[0]['lr']
            hps.append(_lib.member_hparams(d.scale_coeff, d.ham_offset, d.ham_coeff, lr, d.ham_pauli))
        g = self.members[0].trainer.optimizer.param_groups[0]
        _lib.model_sweep_train_steps(self.desc, hps, bounds, gbs, inputs[0], inputs[1] if len(inputs) > 1 else None, out,
                                     self.params, rows, self.exp_avg, self.exp_avg_sq, first_step, g['betas'][0],
                                     g['betas'][1], g['eps'], g['weight_decay'], ham_diag=self.ham_diag)
