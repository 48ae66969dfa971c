"""
Circuit runs per second of the noisy forward (qhea_model_forward_noisy) against the ideal forward (qhea_model_forward_chunks):
  (a) ibm_inference.py's workload: the Antideriv Q2 Net5-1-5-1 model, 100 rows x 10^4 shots;
  (b) Q5 Net20-2-10-2 (the paper's default), 10^4 rows x 10^3 trajectories, expectation mode and shot mode;
  (c) the ideal forward at the same shapes (one evaluation per row).
Each configuration is also run with p1 = p2 = 0 (no random numbers drawn, no error frames): the difference is what the noise
machinery costs.  Times: CUDA events around one host call, 2 warm-up calls, median of `--reps`.
    python scripts/noisy_eval_rate.py [--out profiles/r12_noisy_eval_rate.json] [--only a|b]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quanonet_amd import _lib                               # noqa: E402
from quanonet_amd.models import QuanONetPT                  # noqa: E402
from quanonet_amd.noise import NoiseModel, noisy_predict    # noqa: E402


def _model(n, net, b_in, dev, seed=0):
    torch.manual_seed(seed)
    m = QuanONetPT(n, b_in, 1, net, scale_coeff=0.1, if_trainable_freq=True).double().to(dev)
    with torch.no_grad():
        for p in m.parameters():
            p.uniform_(-1.0, 1.0)
    return m


def _inputs(rows, b_in, dev):
    rng = np.random.default_rng(1)
    return (torch.tensor(rng.uniform(-1, 1, (rows, b_in)), device=dev), torch.tensor(rng.uniform(0, 1, (rows, 1)), device=dev))


def _time(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def noisy_case(name, m, ins, noise, reps):
    rows = ins[0].shape[0]
    runs = rows * (noise.shots or noise.trajectories)
    med, lo, hi = _time(lambda: noisy_predict(m, ins, noise, chunk_rows=rows), reps)
    return {'case': name, 'rows': rows, 'values_per_row': noise.shots or noise.trajectories, 'noise': noise.asdict(),
            'seconds_median': med, 'seconds_min': lo, 'seconds_max': hi, 'circuit_runs_per_s': runs / med}


def ideal_case(name, m, ins, reps):
    rows = ins[0].shape[0]
    desc, flat = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    med, lo, hi = _time(lambda: _lib.model_forward_chunks(desc, ins[0], ins[1], flat, 16384), reps)
    return {'case': name, 'rows': rows, 'seconds_median': med, 'seconds_min': lo, 'seconds_max': hi,
            'evaluations_per_s': rows / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r12_noisy_eval_rate.json'))
    ap.add_argument('--only', choices=['a', 'b'], default=None)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    noisy = dict(p1=1e-3, p2=1e-2, readout=1e-2, seed=7)
    res = []
    if args.only in (None, 'a'):
        m, ins = _model(2, (5, 1, 5, 1), 10, dev), _inputs(100, 10, dev)
        res.append(noisy_case('a: Q2 Net5-1-5-1, 100 rows x 1e4 shots', m, ins, NoiseModel(shots=10000, **noisy), args.reps))
        res.append(noisy_case('a: same, p1 = p2 = 0', m, ins, NoiseModel(shots=10000, readout=1e-2, seed=7), args.reps))
        res.append(ideal_case('c: ideal Q2 Net5-1-5-1, 100 rows', m, ins, args.reps))
    if args.only in (None, 'b'):
        m, ins = _model(5, (20, 2, 10, 2), 100, dev), _inputs(10000, 100, dev)
        res.append(noisy_case('b: Q5 Net20-2-10-2, 1e4 rows x 1e3 trajectories (expectation)', m, ins,
                              NoiseModel(trajectories=1000, **noisy), args.reps))
        res.append(noisy_case('b: Q5 Net20-2-10-2, 1e4 rows x 1e3 shots', m, ins, NoiseModel(shots=1000, **noisy), args.reps))
        res.append(noisy_case('b: expectation, p1 = p2 = 0', m, ins, NoiseModel(trajectories=1000, readout=1e-2, seed=7),
                              args.reps))
        res.append(noisy_case('b: shots, p1 = p2 = 0', m, ins, NoiseModel(shots=1000, readout=1e-2, seed=7), args.reps))
        res.append(ideal_case('c: ideal Q5 Net20-2-10-2, 1e4 rows', m, ins, args.reps))
    for r in res:
        print(json.dumps(r), flush=True)
    if args.only is None:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': 'CUDA events around one host call (prep + trajectory kernel + finish), 2 warm-up calls, median of '
                         f'{args.reps}; circuit runs = rows x trajectories (or shots); ideal = qhea_model_forward_chunks',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
