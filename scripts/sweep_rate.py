"""
Wall time of an ablation grid trained three ways, at reproduce_hamiltonian.sh Exp. 2's shape: QuanONet Q5 Net20-2-10-2,
trainable frequency, batch 100, ham_bound +-1 .. +-10 x 5 seeds = 50 runs, synthetic data, checkpoints off.

    python scripts/sweep_rate.py --rows 10000 --epochs 4 --warmup 1 --seq-runs 5 --out profiles/r06_sweep_rate.json

* sweep:      one SweepSolver over all 50 runs (qhea_model_sweep_train_steps, one launch per kernel and step);
* ensembles:  ten EnsembleSolvers of 5 seeds (one per bound), one after another;
* sequential: PTSolver runs one after another.  Only --seq-runs of them are timed; the 50-run time is that scaled by
              50 / seq-runs (stated in the output as `sequential_scaled_from_runs`).
Each way's epoch time is (time of `epochs` epochs - time of `warmup` epochs) / (epochs - warmup), both measured between device
synchronisations after an untimed one-epoch run; samples/s = runs x rows / epoch time.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BOUNDS = list(range(1, 11))
SEEDS = list(range(5))


def _data(rows, seed=0):
    rng = np.random.default_rng(seed)
    return {'train_branch_input': rng.normal(size=(rows, 100)), 'train_trunk_input': rng.uniform(size=(rows, 2)),
            'train_output': rng.normal(scale=0.5, size=(rows, 1)), 'test_branch_input': rng.normal(size=(8, 100)),
            'test_trunk_input': rng.uniform(size=(8, 2)), 'test_output': rng.normal(size=(8, 1))}


def _cfg(epochs, bound, seed, prefix):
    return {'model_type': 'QuanONet', 'operator': 'Exp2', 'num_qubits': 5, 'net_size': [20, 2, 10, 2], 'scale_coeff': 0.01,
            'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': 100, 'num_epochs': epochs, 'if_save': False,
            'ham_bound': [-bound, bound], 'seed': seed, 'run_id': f'b{bound}_s{seed}', 'prefix': prefix}


def _timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=10000)
    ap.add_argument('--epochs', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seq-runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.solver import PTSolver, set_random_seed
    from quanonet_amd.sweep import SweepSolver
    dev = torch.device('cuda', 0)
    data = _data(a.rows)
    tmp = tempfile.mkdtemp()
    quiet = lambda *x, **k: None
    runs = [(b, s) for b in BOUNDS for s in SEEDS]

    def sweep(ep):
        SweepSolver([_cfg(ep, b, s, tmp) for b, s in runs], data, device=dev, log=quiet).train()

    def ensembles(ep):
        for b in BOUNDS:
            EnsembleSolver([_cfg(ep, b, s, tmp) for s in SEEDS], data, device=dev, log=quiet).train()

    def sequential(ep):
        for b, s in runs[:a.seq_runs]:
            set_random_seed(s)
            PTSolver(_cfg(ep, b, s, tmp), data, device=dev, log=quiet).train()

    timed = a.epochs - a.warmup
    res = {'shape': 'QuanONet Q5 Net20-2-10-2 trainable frequency (reproduce_hamiltonian.sh Exp. 2)', 'batch': 100,
           'rows': a.rows, 'runs': len(runs), 'epochs_timed': timed, 'device': torch.cuda.get_device_name(dev),
           'sequential_scaled_from_runs': a.seq_runs}
    for name, fn, n_runs in (('sweep', sweep, len(runs)), ('ensembles', ensembles, len(runs)),
                             ('sequential', sequential, a.seq_runs)):
        _timed(lambda: fn(1), dev)                                   # warm-up: module loads, workspace
        dt = (_timed(lambda: fn(a.epochs), dev) - _timed(lambda: fn(a.warmup), dev)) / timed
        scale = len(runs) / n_runs
        res[f'{name}_s_per_epoch_50_runs'] = dt * scale
        res[f'{name}_samples_per_s'] = len(runs) * a.rows / (dt * scale)
        print(json.dumps({name: res[f'{name}_samples_per_s']}), flush=True)
    res['sweep_vs_ensembles'] = res['sweep_samples_per_s'] / res['ensembles_samples_per_s']
    res['sweep_vs_sequential'] = res['sweep_samples_per_s'] / res['sequential_samples_per_s']
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
