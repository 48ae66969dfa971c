"""
Wall time of a scaling grid trained two ways, at reproduce_scaling.sh's QuanONet shape: trainable frequency, Net(hb)-2-(ht)-2,
Q2 hb {50..200} x ht {10..300}, Q3 hb {100, 200} x ht {20..300}, Q4 hb {100, 200} x ht {50, 100}, Q5..Q8 hb 100 x ht
{50, 100}, x 5 seeds = 330 runs; batch 100, synthetic data (100 sensors, 1 trunk input), checkpoints off.

    python scripts/qubit_sweep_rate.py --rows 2000 --epochs 3 --warmup 1 --out profiles/r09_qubit_sweep_rate.json

* qubit_sweep:   one QubitSweepSolver over all runs (qhea_model_qubit_sweep_train_steps);
* depth_sweeps:  one DepthSweepSolver per qubit count over its runs, one after another -- what the grid costs without qubit
                 sweeps.
Each way's epoch time is (time of `epochs` epochs - time of `warmup` epochs) / (epochs - warmup), both measured between device
synchronisations after an untimed one-epoch run; samples/s = runs x rows / epoch time.  --trim keeps the first two ht of the
Q2 / Q3 lists (said so in the output).  --once trains the qubit sweep once (for a profiler run) and prints nothing else.
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

GRID = {2: ([50, 100, 150, 200], [10, 20, 30, 40, 50, 60, 100, 150, 200, 300]),
        3: ([100, 200], [20, 40, 50, 100, 150, 200, 300]),
        4: ([100, 200], [50, 100]),
        5: ([100], [50, 100]), 6: ([100], [50, 100]), 7: ([100], [50, 100]), 8: ([100], [50, 100])}
SEEDS = list(range(5))


def _data(rows, seed=0):
    rng = np.random.default_rng(seed)
    return {'train_branch_input': rng.normal(size=(rows, 100)), 'train_trunk_input': rng.uniform(size=(rows, 1)),
            'train_output': rng.normal(scale=0.5, size=(rows, 1)), 'test_branch_input': rng.normal(size=(8, 100)),
            'test_trunk_input': rng.uniform(size=(8, 1)), 'test_output': rng.normal(size=(8, 1))}


def _cfg(epochs, n, hb, ht, seed, prefix):
    return {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': n, 'net_size': [hb, 2, ht, 2],
            'scale_coeff': 0.01, 'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': 100, 'num_epochs': epochs,
            'if_save': False, 'seed': seed, 'run_id': f'q{n}_hb{hb}_ht{ht}_s{seed}', 'prefix': prefix}


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
    ap.add_argument('--trim', action='store_true')
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    dev = torch.device('cuda', 0)
    data = _data(a.rows)
    tmp = tempfile.mkdtemp()
    quiet = lambda *x, **k: None
    grid = {n: (hb, ht[:2] if a.trim and n <= 3 else ht) for n, (hb, ht) in GRID.items()}
    runs = [(n, hb, ht, s) for n, (hbs, hts) in grid.items() for hb in hbs for ht in hts for s in SEEDS]

    def qubit_sweep(ep):
        QubitSweepSolver([_cfg(ep, *r, tmp) for r in runs], data, device=dev, log=quiet).train()

    def depth_sweeps(ep):
        for n in grid:
            DepthSweepSolver([_cfg(ep, *r, tmp) for r in runs if r[0] == n], data, device=dev, log=quiet).train()

    if a.once:
        qubit_sweep(a.epochs)
        torch.cuda.synchronize(dev)
        return
    timed = a.epochs - a.warmup
    res = {'shape': 'QuanONet Net(hb)-2-(ht)-2 trainable frequency, Q2..Q8 (reproduce_scaling.sh)',
           'grid': {f'Q{n}': {'hb': hb, 'ht': ht} for n, (hb, ht) in grid.items()},
           'trimmed': 'Q2 / Q3 ht lists cut to their first two entries' if a.trim else 'no',
           'seeds': len(SEEDS), 'batch': 100, 'rows': a.rows, 'runs': len(runs), 'epochs_timed': timed,
           'device': torch.cuda.get_device_name(dev)}
    for name, fn in (('qubit_sweep', qubit_sweep), ('depth_sweeps', depth_sweeps)):
        _timed(lambda: fn(1), dev)                                   # warm-up: module loads, workspace
        dt = (_timed(lambda: fn(a.epochs), dev) - _timed(lambda: fn(a.warmup), dev)) / timed
        res[f'{name}_s_per_epoch'] = dt
        res[f'{name}_samples_per_s'] = len(runs) * a.rows / dt
        print(json.dumps({name: dt}), flush=True)
    res['speedup'] = res['depth_sweeps_s_per_epoch'] / res['qubit_sweep_s_per_epoch']
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
