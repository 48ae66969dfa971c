"""
Aggregate training rate of a seed ensemble (quanonet_amd.ensemble.EnsembleSolver) against the same R runs of PTSolver one
after another, at the paper's training shape: QuanONet Q5 Net40-2-20-2, trainable frequency, batch 100.

    python scripts/ensemble_rate.py --members 1 2 4 5 8 15 --rows 10000 --epochs 6 --warmup 2 --out profiles/x.json

Train samples/s = R x rows x timed epochs / seconds, timed between device synchronisations after `warmup` epochs (the
solvers' own epoch loops, checkpoints off).  --baseline 0 skips the PTSolver leg (rocprofv3 runs).
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


def _data(rows, seed=0):
    rng = np.random.default_rng(seed)
    return {'train_branch_input': rng.normal(size=(rows, 100)), 'train_trunk_input': rng.uniform(size=(rows, 2)),
            'train_output': rng.normal(scale=0.5, size=(rows, 1)), 'test_branch_input': rng.normal(size=(8, 100)),
            'test_trunk_input': rng.uniform(size=(8, 2)), 'test_output': rng.normal(size=(8, 1))}


def _cfg(epochs, seed, prefix):
    return {'model_type': 'QuanONet', 'operator': 'Rate', 'num_qubits': 5, 'net_size': [40, 2, 20, 2], 'scale_coeff': 0.01,
            'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': 100, 'num_epochs': epochs, 'if_save': False,
            'seed': seed, 'run_id': f'seed{seed}', 'prefix': prefix}


def _timed(make, dev):
    """seconds of one make().train(), between device synchronisations"""
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    make().train()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, nargs='+', default=[1, 2, 4, 5, 8, 15])
    ap.add_argument('--rows', type=int, default=10000)
    ap.add_argument('--epochs', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--baseline', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.solver import PTSolver, set_random_seed
    dev = torch.device('cuda', 0)
    data = _data(a.rows)
    tmp = tempfile.mkdtemp()
    quiet = lambda *x, **k: None
    res = {'model': 'QuanONet Q5 Net40-2-20-2 trainable frequency', 'batch': 100, 'rows': a.rows, 'epochs_timed': a.epochs - a.warmup,
           'device': torch.cuda.get_device_name(dev), 'runs': []}

    def ens(R, ep):
        return lambda: EnsembleSolver([_cfg(ep, s, tmp) for s in range(R)], data, device=dev, log=quiet)

    def seq(R, ep):
        class Seq:
            def train(self):
                for s in range(R):
                    set_random_seed(s)
                    PTSolver(_cfg(ep, s, tmp), data, device=dev, log=quiet).train()
        return lambda: Seq()

    for R in a.members:
        samples = R * a.rows * (a.epochs - a.warmup)
        rec = {'R': R}
        for name, mk in (('ensemble', ens), ('sequential', seq)):
            if name == 'sequential' and not a.baseline:
                continue
            _timed(mk(R, 1), dev)                                   # warm-up: module loads, workspace
            dt = _timed(mk(R, a.epochs), dev) - _timed(mk(R, a.warmup), dev)
            rec[f'{name}_samples_per_s'] = samples / dt
            rec[f'{name}_us_per_step'] = 1e6 * dt / ((a.epochs - a.warmup) * int(np.ceil(a.rows / 100)))
        res['runs'].append(rec)
        print(json.dumps(rec), flush=True)
    base = next((r for r in res['runs'] if r['R'] == 1), None)
    if base:
        for r in res['runs']:
            r['ensemble_vs_R1'] = r['ensemble_samples_per_s'] / base['ensemble_samples_per_s']
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps({r['R']: round(r.get('ensemble_vs_R1', 0), 2) for r in res['runs']}))


if __name__ == '__main__':
    main()
