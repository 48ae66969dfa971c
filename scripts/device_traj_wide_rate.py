"""
Time of the workgroup-resident quantum-jump trajectory call under a device noise model (qhea_model_forward_noisy_device_wide,
n = 10..12) beside the uniform trajectory call (qhea_model_forward_noisy_wide) with the same shape and counts in the same run,
and their ratio:
  (a) Q10 Net10-2-10-2, 1000 rows x 100 trajectories;
  (b) Q12 Net40-2-20-2 (the cfg 5 model), 1000 rows x 64 trajectories.
T of (b): the uniform call runs cfg 5 at 0.39 M trajectories/s; the static instruction counts and barriers of one
sub-layer (profiles/r26_isa_counts.txt) predict 5.3 x that time per trajectory, so 0.074 M/s, and one call is to stay under
2 s: T <= 147, and one full tile per row (64) leaves room for the 1.5 x by which a measured ratio may exceed its prediction.
The device setting has every wire different (rates, T1 / T2, asymmetric readout) and the idle decay on, so every one of the
3 n sites of a sub-layer has gamma > 0 and pays its reduction.  Times: CUDA events around one host call, 2 warm-up calls, median
of `--reps`.
    python scripts/device_traj_wide_rate.py [--out profiles/r26_device_traj_wide_rate.json] [--only a|b]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quanonet_amd.noise import NoiseModel, Sampling, device_noisy_predict, noisy_predict             # noqa: E402
from scripts.device_noise_rate import device_noise                                                   # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                                           # noqa: E402

CASES = {'a': ('a: Q10 Net10-2-10-2, 1000 rows x 100 trajectories', 10, (10, 2, 10, 2), 100, 1000, 100, 4.4),
         'b': ('b: Q12 Net40-2-20-2 (cfg 5), 1000 rows x 64 trajectories', 12, (40, 2, 20, 2), 100, 1000, 64, 5.3)}


def case(key, reps, dev):
    name, n, net, b_in, rows, traj, predicted = CASES[key]
    m, ins = _model(n, net, b_in, dev), _inputs(rows, b_in, dev)
    dn = dataclasses.replace(device_noise(n), idle=True)
    sp = Sampling(trajectories=traj, seed=0)
    nm = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2, trajectories=traj, seed=0)
    out = {'case': name, 'rows': rows, 'values_per_row': traj, 'noise': dn.asdict()}
    med, lo, hi = _time(lambda: device_noisy_predict(m, ins, dn, sp, chunk_rows=rows), reps)
    out['device'] = {'seconds_median': med, 'seconds_min': lo, 'seconds_max': hi, 'circuits_per_s': rows * traj / med}
    med_u, lo, hi = _time(lambda: noisy_predict(m, ins, nm, chunk_rows=rows), reps)
    out['uniform'] = {'seconds_median': med_u, 'seconds_min': lo, 'seconds_max': hi, 'circuits_per_s': rows * traj / med_u}
    out['device_over_uniform'] = med / med_u
    out['predicted_ratio'] = predicted
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r26_device_traj_wide_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.reps, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'CUDA events around one host call, 2 warm-up calls, median of {args.reps}; device = prep + table kernel + '
                         'trajectory kernel + finish under a DeviceNoise with every wire different and idle decay on; uniform = '
                         'noisy_predict under NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2) with the same rows and counts; one host '
                         'call each (chunk_rows = rows); predicted_ratio from profiles/r26_isa_counts.txt',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
