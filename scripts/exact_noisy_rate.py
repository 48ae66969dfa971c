"""
Rows per second of the exact noisy forward (qhea_model_forward_noisy_exact) beside the trajectory call
(qhea_model_forward_noisy, T = 1000 trajectories) and the ideal forward (qhea_model_forward_chunks), same rows, same run:
  (a) ibm_inference.py's workload: the Antideriv-shaped Q2 Net5-1-5-1 model, 100 rows;
  (b) Q5 Net20-2-10-2 (the paper's default), 10^4 rows;
  (c) Q6 Net20-2-10-2, 10^4 rows.
From these the cross-over T* = (time of the exact call) / (time of the trajectory call per trajectory): the trajectory count
above which the exact value is the cheaper one.  Times: CUDA events around one host call, 2 warm-up calls, median of `--reps`.
    python scripts/exact_noisy_rate.py [--out profiles/r13_exact_noisy_rate.json] [--only a|b|c] [--exact-only]
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

from quanonet_amd import _lib                                                    # noqa: E402
from quanonet_amd.noise import NoiseModel, exact_noisy_predict, noisy_predict    # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402

CASES = {'a': ('a: Q2 Net5-1-5-1, 100 rows', 2, (5, 1, 5, 1), 10, 100),
         'b': ('b: Q5 Net20-2-10-2, 1e4 rows', 5, (20, 2, 10, 2), 100, 10000),
         'c': ('c: Q6 Net20-2-10-2, 1e4 rows', 6, (20, 2, 10, 2), 100, 10000)}
TRAJECTORIES = 1000


def case(key, reps, exact_only, dev):
    name, n, net, b_in, rows = CASES[key]
    m, ins = _model(n, net, b_in, dev), _inputs(rows, b_in, dev)
    noise = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2, trajectories=TRAJECTORIES, seed=7)
    out = {'case': name, 'rows': rows, 'noise': noise.asdict()}
    med, lo, hi = _time(lambda: exact_noisy_predict(m, ins, noise, chunk_rows=rows), reps)
    out['exact'] = {'seconds_median': med, 'seconds_min': lo, 'seconds_max': hi, 'rows_per_s': rows / med}
    if exact_only:
        return out
    med_t, lo, hi = _time(lambda: noisy_predict(m, ins, noise, chunk_rows=rows), reps)
    out['trajectories'] = {'values_per_row': TRAJECTORIES, 'seconds_median': med_t, 'seconds_min': lo, 'seconds_max': hi,
                           'circuit_runs_per_s': rows * TRAJECTORIES / med_t}
    desc, flat = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    med_i, lo, hi = _time(lambda: _lib.model_forward_chunks(desc, ins[0], ins[1], flat, 16384), reps)
    out['ideal'] = {'seconds_median': med_i, 'seconds_min': lo, 'seconds_max': hi, 'evaluations_per_s': rows / med_i}
    out['crossover_trajectories'] = med / (med_t / TRAJECTORIES)
    out['exact_over_ideal'] = med / med_i
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r13_exact_noisy_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--exact-only', action='store_true', help='time the exact call alone (profiling runs)')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.reps, args.exact_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and not args.exact_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': 'CUDA events around one host call, 2 warm-up calls, median of '
                         f'{args.reps}; exact = prep + density-matrix kernel; trajectories = prep + trajectory kernel + finish at '
                         f'T = {TRAJECTORIES}; ideal = qhea_model_forward_chunks; crossover_trajectories = exact seconds / '
                         '(trajectory seconds / T)',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
