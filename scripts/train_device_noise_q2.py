#!/usr/bin/env python3
"""
What training under a calibrated device model buys: Antideriv QuanONet Q2 Net5-1-5-1 (the model and training set of
scripts/train_antideriv_q2.py, PyTorch-class initialisation) trained twice per seed -- on the ideal circuit and with
train_device_noise = DeviceNoise.from_calibration(tests/golden/device_calibration_5q.json, [0, 1]) -- and each result scored
twice on the README demo's test set: ideal (PTSolver.evaluate) and under the device (evaluate_noisy(exact=True)).  A 2 x 2 table
per seed and its means, reported as they fall (scripts/train_noise_aware_q2.py is the same under the three-number NoiseModel).

    python scripts/train_device_noise_q2.py [--epochs 1000] [--seeds 0 1 2 3 4] [--out profiles/r23_device_noise_accuracy.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quanonet_amd.noise import DeviceNoise                                       # noqa: E402
from scripts.train_antideriv_q2 import antideriv_data                            # noqa: E402

WIRES = [0, 1]


def device_noise():
    with open(os.path.join(ROOT, 'tests', 'golden', 'device_calibration_5q.json')) as f:
        return DeviceNoise.from_calibration(json.load(f), WIRES)


def run(seed, epochs, noise, data, device, prefix):
    """one training run (noise: the DeviceNoise to train under, or None), scored ideal and under the device"""
    from quanonet_amd.solver import PTSolver, set_random_seed
    arm = 'ideal' if noise is None else 'device'
    cfg = {'model_type': 'QuanONet', 'operator': 'Antideriv', 'num_qubits': 2, 'net_size': [5, 1, 5, 1],
           'scale_coeff': 0.001, 'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': 100,
           'num_epochs': epochs, 'prefix': prefix, 'run_id': f'{arm}_seed{seed}', 'seed': seed}
    if noise is not None:
        cfg['train_device_noise'] = noise.asdict()
    set_random_seed(seed)
    s = PTSolver(cfg, data, device=device, log=lambda *a, **k: None)
    t0 = time.perf_counter()
    hist = s.train()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ideal = s.evaluate(None)
    noisy = s.evaluate_noisy(device_noise(), exact=True)
    steps = epochs * int(np.ceil(data['train_output'].shape[0] / 100))
    return {'seed': seed, 'trained': 'under the device' if noise is not None else 'ideal',
            'scored_ideal': {k: ideal[k] for k in ('rel_l2', 'MSE', 'MAE')},
            'scored_device': {k: noisy[k] for k in ('rel_l2', 'MSE', 'MAE')},
            'best_train_mse': float(min(hist['loss_train'])), 'train_seconds': dt, 'us_per_step': 1e6 * dt / steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=1000)
    ap.add_argument('--seeds', type=int, nargs='*', default=[0, 1, 2, 3, 4])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    data = antideriv_data()
    dn = device_noise()
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for noise in (None, dn):
            for seed in a.seeds:
                runs.append(run(seed, a.epochs, noise, data, dev, tmp))
                print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for arm in ('ideal', 'under the device'):
        rs = [r for r in runs if r['trained'] == arm]
        summary[f'trained {arm}'] = {f'{col} {k}': {'mean': float(np.mean([r[col][k] for r in rs])),
                                                   'std': float(np.std([r[col][k] for r in rs]))}
                                     for col in ('scored_ideal', 'scored_device') for k in ('rel_l2', 'MSE')}
    doc = {'what': 'Antideriv QuanONet Q2 Net5-1-5-1 S0.001 TF trained from scratch (fp64, reference hyper-parameters) on the ideal '
                   'circuit and under DeviceNoise.from_calibration(tests/golden/device_calibration_5q.json, [0, 1]); each scored '
                   'ideal and under the device (exact) on the README demo test set',
           'noise': dn.asdict(), 'wires': WIRES, 'epochs': a.epochs, 'runs': runs, 'summary': summary}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
