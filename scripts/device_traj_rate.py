"""
Time of the quantum-jump trajectory call under a device noise model (qhea_model_forward_noisy_device) beside the uniform
trajectory call (qhea_model_forward_noisy / ..._wide) with the same shape and counts in the same run, and their ratio:
  (a) Q2 Net5-1-5-1, 100 rows x 10^4 shots (ibm_inference.py's workload);
  (b) Q5 Net20-2-10-2, 1000 rows x 100 trajectories;
  (c) HEAQNN Q8 depth 20 x 2 on 102 inputs (the cfg 4 model), 1000 rows x 100 trajectories;
  (d) Q9 Net2-1-2-1 (the smallest depth), 1000 rows x 100 trajectories.
(a) and (b) also time the exact call under the same DeviceNoise.  The device setting has every wire different (rates, T1 / T2,
asymmetric readout) and the idle decay on.  Times: CUDA events around one host call, 2 warm-up calls, median of `--reps`.
    python scripts/device_traj_rate.py [--out profiles/r24_device_traj_rate.json] [--only a|b|c|d]
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

from quanonet_amd.models import HEAQNNPT                                                             # noqa: E402
from quanonet_amd.noise import NoiseModel, Sampling, device_noisy_predict, exact_noisy_predict, noisy_predict   # noqa: E402
from scripts.device_noise_rate import device_noise                                                   # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                                           # noqa: E402

CASES = {'a': ('a: Q2 Net5-1-5-1, 100 rows x 10000 shots', 'quanonet', 2, (5, 1, 5, 1), 10, 100, 10000, 0, True),
         'b': ('b: Q5 Net20-2-10-2, 1000 rows x 100 trajectories', 'quanonet', 5, (20, 2, 10, 2), 100, 1000, 0, 100, True),
         'c': ('c: HEAQNN Q8 depth 20 x 2, input 102, 1000 rows x 100 trajectories', 'heaqnn', 8, (20, 2), 102, 1000, 0, 100, False),
         'd': ('d: Q9 Net2-1-2-1, 1000 rows x 100 trajectories', 'quanonet', 9, (2, 1, 2, 1), 10, 1000, 0, 100, False)}


def case(key, reps, dev):
    name, kind, n, net, b_in, rows, shots, traj, exact = CASES[key]
    if kind == 'heaqnn':
        torch.manual_seed(0)
        m = HEAQNNPT(n, b_in, net, scale_coeff=0.1, if_trainable_freq=True).double().to(dev)
        ins = _inputs(rows, b_in, dev)[:1]
    else:
        m, ins = _model(n, net, b_in, dev), _inputs(rows, b_in, dev)
    dn = dataclasses.replace(device_noise(n), idle=True)
    count = shots if shots else traj
    sp = Sampling(shots=shots, trajectories=max(traj, 1), seed=0)
    nm = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2, shots=shots, trajectories=max(traj, 1), seed=0)
    out = {'case': name, 'rows': rows, 'values_per_row': count, 'noise': dn.asdict()}
    med, lo, hi = _time(lambda: device_noisy_predict(m, ins, dn, sp, chunk_rows=rows), reps)
    out['device'] = {'seconds_median': med, 'seconds_min': lo, 'seconds_max': hi, 'circuits_per_s': rows * count / med}
    med_u, lo, hi = _time(lambda: noisy_predict(m, ins, nm, chunk_rows=rows), reps)
    out['uniform'] = {'seconds_median': med_u, 'seconds_min': lo, 'seconds_max': hi, 'circuits_per_s': rows * count / med_u}
    out['device_over_uniform'] = med / med_u
    if exact:
        med_e, lo, hi = _time(lambda: exact_noisy_predict(m, ins, dn, chunk_rows=rows), reps)
        out['exact'] = {'seconds_median': med_e, 'seconds_min': lo, 'seconds_max': hi, 'rows_per_s': rows / med_e}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r24_device_traj_rate.json'))
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
                         'call each (chunk_rows = rows)',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
