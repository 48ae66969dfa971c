"""
Time per training step under a device noise model (qhea_model_train_steps_noisy_device_exact) beside, on the same rows and in
the same run, the uniform noise-aware step (qhea_model_train_steps_noisy_exact), and their ratio:
  (a) Q2 Net5-1-5-1, batch 100;
  (b) Q5 Net20-2-10-2, batch 100;   (c) the same, batch 1000;
  (d) Q6 Net20-2-10-2, batch 100.
The device setting is scripts/device_noise_rate.py's (every wire different, idle decay on); the kernel's work does not depend
on the values.  Times: device events around ONE train_steps call of `--steps` steps, 2 warm-up calls, median of `--reps`;
reported per step.  The device call launches its table kernel once per call, so 1 / steps of it is in every step.
    python scripts/device_noise_training_rate.py [--out profiles/r23_device_noise_training_rate.json] [--only a|b|c|d] [--device-only]
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
from quanonet_amd.noise import NoiseModel, amplification, device_amplification   # noqa: E402
from scripts.device_noise_rate import device_noise                               # noqa: E402
from scripts.noise_aware_rate import CASES                                       # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402


def case(key, steps, reps, device_only, dev):
    name, n, net, b_in, batch = CASES[key]
    m = _model(n, net, b_in, dev)
    rows = steps * batch
    ins = _inputs(rows, b_in, dev)
    y = torch.tensor(np.random.default_rng(2).normal(scale=0.5, size=rows), device=dev)
    dn, uniform = device_noise(n), NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2)
    desc, flat0 = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    P = flat0.numel()
    bounds, sizes = [i * batch for i in range(steps + 1)], [batch] * steps
    out = torch.zeros(steps, P + 2, dtype=torch.float64, device=dev)
    res = {'case': name, 'batch': batch, 'steps_per_call': steps, 'parameters': P, 'noise': dn.asdict(),
           'log10_amplification_device': device_amplification(m, dn), 'log10_amplification_uniform': amplification(m, uniform)}

    def state():
        return flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0)

    p, mm, vv = state()
    rec = dn.params(n)
    device = lambda: _lib.model_train_steps_noisy_device_exact(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-4,
                                                               0.9, 0.999, 1e-8, 0.0, rec)
    med, lo, hi = _time(device, reps)
    res['device_step'] = {'seconds_median': med / steps, 'seconds_min': lo / steps, 'seconds_max': hi / steps}
    if device_only:
        return res
    p2, m2, v2 = state()
    nz = uniform.params()
    aware = lambda: _lib.model_train_steps_noisy_exact(desc, bounds, sizes, ins[0], ins[1], y, p2, out, m2, v2, 1, 1e-4, 0.9, 0.999,
                                                       1e-8, 0.0, nz)
    med_u, lo, hi = _time(aware, reps)
    res['uniform_step'] = {'seconds_median': med_u / steps, 'seconds_min': lo / steps, 'seconds_max': hi / steps}
    res['device_over_uniform'] = med / med_u
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r23_device_noise_training_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--device-only', action='store_true', help='time the device-noise call alone (profiling runs)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.steps, args.reps, args.device_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and not args.device_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call of {args.steps} steps, 2 warm-up calls, median of {args.reps}, per '
                         'step; device step = (table kernel once per call) + prep + density_dev_bwd_kernel + reduce/Adam under a '
                         'DeviceNoise with every wire different and idle decay on; uniform step = prep + density_bwd_kernel + '
                         'reduce/Adam under NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2); both on the same rows',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
