"""
Wall time of a capacity grid trained two ways, at reproduce_capacity.sh's shape: QuanONet Q2 Net(hb)-2-(ht)-2, trainable
frequency, batch 100, hb in {50, 100, 150, 200} x ht in {10, 50, 100, 300} x 5 seeds = 80 runs, synthetic data, checkpoints off.

    python scripts/depth_sweep_rate.py --rows 2000 --epochs 3 --warmup 1 --out profiles/r08_depth_sweep_rate.json

* depth_sweep:  one DepthSweepSolver over all runs (qhea_model_depth_sweep_train_steps, one launch per kernel and step);
* sweeps:       one SweepSolver per (hb, ht) shape over its 5 seeds, one after another -- what the grid costs without
                depth sweeps (these shapes are outside the ZYZ kernels, so each of them runs as R single-model calls).
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

HB = [50, 100, 150, 200]
HT = [10, 50, 100, 300]
SEEDS = list(range(5))


def _data(rows, seed=0):
    rng = np.random.default_rng(seed)
    return {'train_branch_input': rng.normal(size=(rows, 100)), 'train_trunk_input': rng.uniform(size=(rows, 1)),
            'train_output': rng.normal(scale=0.5, size=(rows, 1)), 'test_branch_input': rng.normal(size=(8, 100)),
            'test_trunk_input': rng.uniform(size=(8, 1)), 'test_output': rng.normal(size=(8, 1))}


def _cfg(epochs, hb, ht, seed, prefix):
    return {'model_type': 'QuanONet', 'operator': 'Capacity', 'num_qubits': 2, 'net_size': [hb, 2, ht, 2], 'scale_coeff': 0.01,
            'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': 100, 'num_epochs': epochs, 'if_save': False,
            'seed': seed, 'run_id': f'hb{hb}_ht{ht}_s{seed}', 'prefix': prefix}


def _timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=2000)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.sweep import SweepSolver
    dev = torch.device('cuda', 0)
    data = _data(a.rows)
    tmp = tempfile.mkdtemp()
    quiet = lambda *x, **k: None
    shapes = [(hb, ht) for hb in HB for ht in HT]
    runs = [(hb, ht, s) for hb, ht in shapes for s in SEEDS]

    def depth_sweep(ep):
        DepthSweepSolver([_cfg(ep, hb, ht, s, tmp) for hb, ht, s in runs], data, device=dev, log=quiet).train()

    def sweeps(ep):
        for hb, ht in shapes:
            SweepSolver([_cfg(ep, hb, ht, s, tmp) for s in SEEDS], data, device=dev, log=quiet).train()

    timed = a.epochs - a.warmup
    res = {'shape': 'QuanONet Q2 Net(hb)-2-(ht)-2 trainable frequency (reproduce_capacity.sh)', 'hb': HB, 'ht': HT,
           'seeds': len(SEEDS), 'batch': 100, 'rows': a.rows, 'runs': len(runs), 'epochs_timed': timed,
           'device': torch.cuda.get_device_name(dev)}
    for name, fn in (('depth_sweep', depth_sweep), ('sweeps', sweeps)):
        _timed(lambda: fn(1), dev)                                   # warm-up: module loads, workspace
        dt = (_timed(lambda: fn(a.epochs), dev) - _timed(lambda: fn(a.warmup), dev)) / timed
        res[f'{name}_s_per_epoch'] = dt
        res[f'{name}_samples_per_s'] = len(runs) * a.rows / dt
        print(json.dumps({name: dt}), flush=True)
    res['speedup'] = res['sweeps_s_per_epoch'] / res['depth_sweep_s_per_epoch']
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
