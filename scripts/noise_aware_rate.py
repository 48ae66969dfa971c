"""
Time per training step of noise-aware training (qhea_model_train_steps_noisy_exact) beside, on the same rows and in the same
run, the exact noisy forward (qhea_model_forward_noisy_exact) and the ideal training step (qhea_model_train_steps):
  (a) Q2 Net5-1-5-1, batch 100 (the Antideriv model of the reference's shipped checkpoint);
  (b) Q5 Net20-2-10-2, batch 100 (the paper's batch);   (c) the same, batch 1000;
  (d) Q6 Net20-2-10-2, batch 100.
Noise: p1 = 1e-3, p2 = 1e-2, readout = 1e-2.  Times: device events around ONE train_steps call of `--steps` steps (the forward:
around `--steps` calls), 2 warm-up calls, median of `--reps`; reported per step.
    python scripts/noise_aware_rate.py [--out profiles/r14_noise_aware_rate.json] [--only a|b|c|d] [--aware-only]
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
from quanonet_amd.noise import NoiseModel, amplification                         # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402

CASES = {'a': ('a: Q2 Net5-1-5-1, batch 100', 2, (5, 1, 5, 1), 10, 100),
         'b': ('b: Q5 Net20-2-10-2, batch 100', 5, (20, 2, 10, 2), 100, 100),
         'c': ('c: Q5 Net20-2-10-2, batch 1000', 5, (20, 2, 10, 2), 100, 1000),
         'd': ('d: Q6 Net20-2-10-2, batch 100', 6, (20, 2, 10, 2), 100, 100)}


def case(key, steps, reps, aware_only, dev):
    name, n, net, b_in, batch = CASES[key]
    m = _model(n, net, b_in, dev)
    rows = steps * batch
    ins = _inputs(rows, b_in, dev)
    y = torch.tensor(np.random.default_rng(2).normal(scale=0.5, size=rows), device=dev)
    noise = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2)
    desc, flat0 = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    P = flat0.numel()
    bounds, sizes = [i * batch for i in range(steps + 1)], [batch] * steps
    out = torch.zeros(steps, P + 2, dtype=torch.float64, device=dev)
    res = {'case': name, 'batch': batch, 'steps_per_call': steps, 'parameters': P, 'noise': noise.asdict(),
           'log10_amplification': amplification(m, noise)}

    def state():
        return flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0)

    p, mm, vv = state()
    nz = noise.params()
    aware = lambda: _lib.model_train_steps_noisy_exact(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-4, 0.9, 0.999,
                                                       1e-8, 0.0, nz)
    med, lo, hi = _time(aware, reps)
    res['noise_aware_step'] = {'seconds_median': med / steps, 'seconds_min': lo / steps, 'seconds_max': hi / steps}
    if aware_only:
        return res
    pred = torch.empty(batch, dtype=torch.float64, device=dev)

    def forward():
        for i in range(steps):
            _lib.model_forward_noisy_exact(desc, ins[0][bounds[i]:bounds[i + 1]], ins[1][bounds[i]:bounds[i + 1]], flat0, nz, out=pred)
    med_f, lo, hi = _time(forward, reps)
    res['exact_forward'] = {'seconds_median': med_f / steps, 'seconds_min': lo / steps, 'seconds_max': hi / steps}
    p2, m2, v2 = state()
    ideal = lambda: _lib.model_train_steps(desc, bounds, sizes, ins[0], ins[1], y, p2, out, m2, v2, 1, 1e-4, 0.9, 0.999, 1e-8, 0.0)
    med_i, lo, hi = _time(ideal, reps)
    res['ideal_step'] = {'seconds_median': med_i / steps, 'seconds_min': lo / steps, 'seconds_max': hi / steps}
    res['aware_over_forward'] = med / med_f
    res['aware_over_ideal'] = med / med_i
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r14_noise_aware_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--aware-only', action='store_true', help='time the noise-aware call alone (profiling runs)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.steps, args.reps, args.aware_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and not args.aware_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call of {args.steps} steps (exact forward: {args.steps} calls), 2 warm-up '
                         f'calls, median of {args.reps}, per step; noise-aware step = prep + density backward + reduce/Adam; exact '
                         'forward = prep + density forward; ideal step = qhea_model_train_steps',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
