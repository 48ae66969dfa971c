"""
Time of the exact noisy forward under a device noise model (qhea_model_forward_noisy_device_exact) beside the uniform exact
call (qhea_model_forward_noisy_exact) on the same rows in the same run, and their ratio:
  (a) Q2 Net5-1-5-1, 100 rows (ibm_inference.py's workload);
  (b) Q5 Net20-2-10-2, 100 rows;  (c) the same, 1000 rows;
  (d) Q6 Net20-2-10-2, 100 rows.
The device setting has every wire different (rates, T1 / T2, asymmetric readout) and the idle decay on; the kernel's work does
not depend on the values.  Times: CUDA events around one host call, 2 warm-up calls, median of `--reps`.
    python scripts/device_noise_rate.py [--out profiles/r19_device_noise_rate.json] [--only a|b|c|d] [--device-only]
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

from quanonet_amd.noise import DeviceNoise, NoiseModel, exact_noisy_predict      # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402

CASES = {'a': ('a: Q2 Net5-1-5-1, 100 rows', 2, (5, 1, 5, 1), 10, 100),
         'b': ('b: Q5 Net20-2-10-2, 100 rows', 5, (20, 2, 10, 2), 100, 100),
         'c': ('c: Q5 Net20-2-10-2, 1000 rows', 5, (20, 2, 10, 2), 100, 1000),
         'd': ('d: Q6 Net20-2-10-2, 100 rows', 6, (20, 2, 10, 2), 100, 100)}


def device_noise(n):
    rng = np.random.default_rng(n)
    t1 = rng.uniform(60e-6, 150e-6, n)
    return DeviceNoise(p1=rng.uniform(2e-4, 1e-3, n), p2=rng.uniform(5e-3, 1.5e-2, n), readout01=rng.uniform(5e-3, 2e-2, n),
                       readout10=rng.uniform(1e-2, 4e-2, n), t1=t1, t2=t1 * rng.uniform(0.5, 1.5, n), t_rx=7e-8, t_rot=7e-8,
                       t_cx=4e-7)


def case(key, reps, device_only, dev):
    name, n, net, b_in, rows = CASES[key]
    m, ins = _model(n, net, b_in, dev), _inputs(rows, b_in, dev)
    dn = device_noise(n)
    out = {'case': name, 'rows': rows, 'noise': dn.asdict()}
    med, lo, hi = _time(lambda: exact_noisy_predict(m, ins, dn, chunk_rows=rows), reps)
    out['device'] = {'seconds_median': med, 'seconds_min': lo, 'seconds_max': hi, 'rows_per_s': rows / med}
    if device_only:
        return out
    uniform = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2)
    med_u, lo, hi = _time(lambda: exact_noisy_predict(m, ins, uniform, chunk_rows=rows), reps)
    out['uniform'] = {'seconds_median': med_u, 'seconds_min': lo, 'seconds_max': hi, 'rows_per_s': rows / med_u}
    out['device_over_uniform'] = med / med_u
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r19_device_noise_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--device-only', action='store_true', help='time the device-noise call alone (profiling runs)')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.reps, args.device_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and not args.device_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'CUDA events around one host call, 2 warm-up calls, median of {args.reps}; device = prep + '
                         'density_dev_fwd_kernel under a DeviceNoise with every wire different and idle decay on; uniform = prep + '
                         'density_fwd_kernel under NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2); both on the same rows, one '
                         'host call each (chunk_rows = rows)',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
