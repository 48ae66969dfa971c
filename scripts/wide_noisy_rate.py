"""
Circuit runs per second of the wide noisy forward (qhea_model_forward_noisy_wide, n = 7..12) against the ideal forward:
  (a) HEAQNN Q8 depth 20 x 2 on 102 inputs (the cfg 4 model)   -- the wave-resident trajectory kernel;
  (b) QuanONet Q10 Net10-2-10-2                                 -- the LDS kernel, one wave per workgroup;
  (c) QuanONet Q12 Net40-2-20-2 (the cfg 5 model)               -- the LDS kernel, 256 threads and 64 KiB of state.
Each workload: 10^3 rows x T trajectories (expectation mode) and 10^3 rows x T shots at p1 = 1e-3, p2 = 1e-2, q = 1e-2, the
same two with p1 = p2 = 0 (no random numbers drawn, no error frames), and the ideal qhea_model_forward on the same rows.
T = 1000 unless a call would take more than `--budget` seconds: a one-tile call (T = 64) is timed first and T is scaled down
to a multiple of 64 that fits; the result says which T ran.  Times: device events around one host call, 2 warm-up calls,
median of `--reps` (scripts/noisy_eval_rate.py's method).
    python scripts/wide_noisy_rate.py [--out profiles/r17_wide_noisy_rate.json] [--only a|b|c] [--values T]
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
from quanonet_amd.models import HEAQNNPT, QuanONetPT        # noqa: E402
from quanonet_amd.noise import NoiseModel, noisy_predict    # noqa: E402
from scripts.noisy_eval_rate import _time                   # noqa: E402

ROWS = 1000
WORKLOADS = {'a': ('HEAQNN Q8 depth 20 x 2, input 102', 'heaqnn', 8, (20, 2), 102, 0),
             'b': ('QuanONet Q10 Net10-2-10-2', 'quanonet', 10, (10, 2, 10, 2), 100, 2),
             'c': ('QuanONet Q12 Net40-2-20-2', 'quanonet', 12, (40, 2, 20, 2), 100, 2)}


def _model(kind, n, net, b_in, t_in, dev):
    torch.manual_seed(0)
    if kind == 'heaqnn':
        m = HEAQNNPT(n, b_in, net, scale_coeff=0.1, if_trainable_freq=True)
    else:
        m = QuanONetPT(n, b_in, t_in, net, scale_coeff=0.1, if_trainable_freq=True)
    m = m.double().to(dev)
    with torch.no_grad():
        for p in m.parameters():
            p.uniform_(-1.0, 1.0)
    rng = np.random.default_rng(1)
    ins = [torch.tensor(rng.uniform(-1, 1, (ROWS, b_in)), device=dev)]
    if kind != 'heaqnn':
        ins.append(torch.tensor(rng.uniform(0, 1, (ROWS, t_in)), device=dev))
    return m, tuple(ins)


def _noisy_case(name, m, ins, noise, reps):
    T = noise.shots or noise.trajectories
    med, lo, hi = _time(lambda: noisy_predict(m, ins, noise, chunk_rows=ROWS), reps)
    return {'case': name, 'rows': ROWS, 'values_per_row': T, 'noise': noise.asdict(), 'seconds_median': med, 'seconds_min': lo,
            'seconds_max': hi, 'circuit_runs_per_s': ROWS * T / med}


def workload(key, dev, reps, budget, values):
    title, kind, n, net, b_in, t_in = WORKLOADS[key]
    m, ins = _model(kind, n, net, b_in, t_in, dev)
    noisy = dict(p1=1e-3, p2=1e-2, readout=1e-2, seed=7)
    T = values
    if T is None:
        tile, _, _ = _time(lambda: noisy_predict(m, ins, NoiseModel(shots=64, **noisy), chunk_rows=ROWS), 1)
        T = 1000 if tile / 64 * 1000 <= budget else max(64, int(budget / (tile / 64)) // 64 * 64)
    res = [_noisy_case(f'{key}: {title}, {ROWS} rows x {T} trajectories (expectation)', m, ins,
                       NoiseModel(trajectories=T, **noisy), reps),
           _noisy_case(f'{key}: {ROWS} rows x {T} shots', m, ins, NoiseModel(shots=T, **noisy), reps),
           _noisy_case(f'{key}: expectation, p1 = p2 = 0', m, ins, NoiseModel(trajectories=T, readout=1e-2, seed=7), reps),
           _noisy_case(f'{key}: shots, p1 = p2 = 0', m, ins, NoiseModel(shots=T, readout=1e-2, seed=7), reps)]
    desc, flat = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    trunk = ins[1] if len(ins) > 1 else None
    med, lo, hi = _time(lambda: _lib.model_forward(desc, ins[0], trunk, flat), reps)
    res.append({'case': f'{key}: ideal qhea_model_forward, {ROWS} rows', 'rows': ROWS, 'seconds_median': med, 'seconds_min': lo,
                'seconds_max': hi, 'evaluations_per_s': ROWS / med})
    ideal = ROWS / med
    for r in res[:4]:
        r['rate_over_ideal'] = r['circuit_runs_per_s'] / ideal
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r17_wide_noisy_rate.json'))
    ap.add_argument('--only', choices=sorted(WORKLOADS), default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--budget', type=float, default=3.0, help='seconds one noisy call may take before T is scaled down')
    ap.add_argument('--values', type=int, default=None, help='trajectories / shots per row (default: 1000, scaled to the budget)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in ([args.only] if args.only else sorted(WORKLOADS)):
        for r in workload(key, dev, args.reps, args.budget, args.values):
            print(json.dumps(r), flush=True)
            res.append(r)
    if args.only is None:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': 'device events around one host call (prep + trajectory kernel + finish), 2 warm-up calls, median of '
                         f'{args.reps}; circuit runs = rows x trajectories (or shots); ideal = qhea_model_forward on the same rows; '
                         'rate_over_ideal = noisy circuit runs/s over ideal evaluations/s (the n = 5 precedent of DESIGN 7f: 0.55 '
                         'per noiseless run)',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
