"""
Wall time of reproduce_circuit.sh's grid trained as one QubitSweepSolver -- QuanONet Net(hb)-2-(ht)-2, trainable frequency,
Q2 hb {50, 100}, Q5 hb {20, 40}, Q10 hb {10, 20}, ht {10, 20, 30, 40}, x 5 seeds = 120 runs; batch 100, synthetic data (100
sensors, 1 trunk input), checkpoints off -- plus a 5-seed Q10 Net20-2-40-2 EnsembleSolver and a 5-seed Q12 Net5-2-5-2 one.

    python scripts/circuit_grid_rate.py --rows 1000 --out profiles/r10_circuit_grid_rate.json
    QHEA_LIB=<parent build>/libquanonet_hea.so python scripts/circuit_grid_rate.py --out ...     (the parent commit's library)

* grid:      the whole grid, one QubitSweepSolver;
* grid_q10:  its 40 Q10 runs alone, one QubitSweepSolver;
* q10_ens:   EnsembleSolver, Q10 Net20-2-40-2, 5 seeds;   q12_ens: EnsembleSolver, Q12 Net5-2-5-2, 5 seeds.
Each case's epoch time is (time of `epochs` epochs - time of one epoch) / (epochs - 1), both measured between device
synchronisations after an untimed one-epoch run; samples/s = runs x rows / epoch time.  --once CASE trains that case for
`epochs` epochs (for a profiler run) and prints nothing else.
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

GRID = {2: [50, 100], 5: [20, 40], 10: [10, 20]}
HT = [10, 20, 30, 40]
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
    ap.add_argument('--rows', type=int, default=1000)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--once', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from quanonet_amd import _lib
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    dev = torch.device('cuda', 0)
    data = _data(a.rows)
    tmp = tempfile.mkdtemp()
    quiet = lambda *x, **k: None
    grid = [(n, hb, ht, s) for n, hbs in GRID.items() for hb in hbs for ht in HT for s in SEEDS]
    cases = {'grid': (QubitSweepSolver, grid),
             'grid_q10': (QubitSweepSolver, [r for r in grid if r[0] == 10]),
             'q10_ens': (EnsembleSolver, [(10, 20, 40, s) for s in SEEDS]),
             'q12_ens': (EnsembleSolver, [(12, 5, 5, s) for s in SEEDS])}

    def train(name, ep):
        cls, runs = cases[name]
        cls([_cfg(ep, *r, tmp) for r in runs], data, device=dev, log=quiet).train()

    if a.once:
        train(a.once, a.epochs)
        torch.cuda.synchronize(dev)
        return
    timed = a.epochs - 1
    res = {'shape': 'QuanONet Net(hb)-2-(ht)-2 trainable frequency (reproduce_circuit.sh)',
           'grid': {f'Q{n}': {'hb': hb, 'ht': HT} for n, hb in GRID.items()}, 'seeds': len(SEEDS), 'batch': 100,
           'rows': a.rows, 'epochs_timed': timed, 'library': os.path.basename(os.path.dirname(_lib.LIB_PATH)) or _lib.LIB_PATH,
           'qhea_version': _lib.load().qhea_version(), 'device': torch.cuda.get_device_name(dev)}
    for name, (cls, runs) in cases.items():
        _timed(lambda: train(name, 1), dev)                          # warm-up: module loads, workspace
        dt = (_timed(lambda: train(name, a.epochs), dev) - _timed(lambda: train(name, 1), dev)) / timed
        res[name] = {'solver': cls.__name__, 'runs': len(runs), 's_per_epoch': dt, 'samples_per_s': len(runs) * a.rows / dt}
        print(json.dumps({name: dt}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
