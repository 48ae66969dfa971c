"""
Time per training step of exact noise-aware training at n = 7..9 (qhea_model_train_steps_noisy_exact_wide: rho and O tiled
through device memory) beside, on the same rows and in the same run, the exact noisy forward it is built on
(qhea_model_forward_noisy_exact_wide) and the sampled-trajectory step (qhea_model_train_steps_noisy_wide at T = 64):
  (a) QuanONet Q7 Net20-2-10-2, batch 100;   (b) HEAQNN Q8 20 x 2, 102 inputs, batch 100 (bench.py's cfg 4 model);
  (c) the same, batch 2048 (cfg 4);           (d) QuanONet Q9 Net20-2-10-2, batch 64.
Noise: p1 = 1e-3, p2 = 1e-2, readout = 1e-2.  Times: device events around ONE train_steps call of `--steps` steps (the forward:
around `--steps` calls), 2 warm-up calls, median of `--reps`; reported per step.  T* is the trajectory count at which the
sampled step costs what the exact step costs (the sampled step's time is proportional to T).
The estimate the ratio step / forward is set beside: a forward stage moves rho once each way, a reverse stage rho and O, so a
step has about 3 x the forward's traffic at half its workgroups per CU: 3 .. 6 x the forward's time.
    python scripts/exact_noisy_wide_training_rate.py [--out profiles/r40_exact_noisy_wide_training_rate.json] [--only a|b|c|d]
                                                     [--exact-only]
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
from quanonet_amd.noise import NoiseModel                                        # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402
from scripts.noisy_traj_training_rate import _heaqnn, _stat                      # noqa: E402

CASES = {'a': ('a: QuanONet Q7 Net20-2-10-2, batch 100', 'quanonet', 7, (20, 2, 10, 2), 100, 100),
         'b': ('b: HEAQNN Q8 20 x 2, 102 inputs, batch 100', 'heaqnn', 8, (20, 2), 102, 100),
         'c': ('c: HEAQNN Q8 20 x 2, 102 inputs, batch 2048', 'heaqnn', 8, (20, 2), 102, 2048),
         'd': ('d: QuanONet Q9 Net20-2-10-2, batch 64', 'quanonet', 9, (20, 2, 10, 2), 100, 64)}
T_SAMPLED = 64


def case(key, steps, reps, exact_only, dev):
    name, kind, n, net, b_in, batch = CASES[key]
    rows = steps * batch
    if kind == 'heaqnn':
        m = _heaqnn(n, net, b_in, dev)
        ins = (_inputs(rows, b_in, dev)[0], None)
    else:
        m = _model(n, net, b_in, dev)
        ins = _inputs(rows, b_in, dev)
    y = torch.tensor(np.random.default_rng(2).normal(scale=0.5, size=rows), device=dev)
    desc, flat0 = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    P = flat0.numel()
    bounds, sizes = [i * batch for i in range(steps + 1)], [batch] * steps
    out = torch.zeros(steps, P + 2, dtype=torch.float64, device=dev)
    noise = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2, trajectories=T_SAMPLED, seed=7)
    nz = noise.params()
    res = {'case': name, 'batch': batch, 'steps_per_call': steps, 'parameters': P, 'noise': noise.asdict(),
           'log10_amplification': _lib.model_exact_noisy_log10_amplification(desc, nz),
           'workspace_bytes': _lib.model_exact_noisy_wide_grad_workspace_bytes(desc, batch),
           'library': os.path.relpath(_lib.LIB_PATH, ROOT)}

    def state():
        return flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0)

    p, mm, vv = state()
    exact = lambda: _lib.model_train_steps_noisy_exact_wide(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-4, 0.9,
                                                            0.999, 1e-8, 0.0, nz)
    t_exact = _time(exact, reps)
    res['exact_step'] = _stat(t_exact, steps)
    if exact_only:
        return res
    pred = torch.empty(batch, dtype=torch.float64, device=dev)

    def forward():
        for i in range(steps):
            a, b = bounds[i], bounds[i + 1]
            _lib.model_forward_noisy_exact_wide(desc, ins[0][a:b], None if ins[1] is None else ins[1][a:b], flat0, nz, out=pred)
    t_fwd = _time(forward, reps)
    res['exact_forward'] = _stat(t_fwd, steps)
    res['step_over_forward'] = t_exact[0] / t_fwd[0]
    res['step_over_forward_estimate'] = '3 .. 6 (3 x the traffic at half the workgroups per CU)'
    p2, m2, v2 = state()
    sampled = lambda: _lib.model_train_steps_noisy_wide(desc, bounds, sizes, ins[0], ins[1], y, p2, out, m2, v2, 1, 1e-4, 0.9,
                                                        0.999, 1e-8, 0.0, nz)
    t_smp = _time(sampled, reps)
    res['sampled_step_T64'] = _stat(t_smp, steps)
    res['T_star'] = T_SAMPLED * t_exact[0] / t_smp[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r40_exact_noisy_wide_training_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--exact-only', action='store_true', help='time the new call alone (profiling runs)')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.steps, args.reps, args.exact_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and not args.exact_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call of {args.steps} steps (exact forward: {args.steps} calls), 2 warm-up '
                         f'calls, median of {args.reps}, per step; exact step = prep + value table + forward stages + read-out + '
                         'O_N + reverse stages + fold + reduce/Adam; exact forward = prep + value table + stages + read-out on the '
                         f'same rows; sampled step = qhea_model_train_steps_noisy_wide at T = {T_SAMPLED}; T* = {T_SAMPLED} x exact '
                         'step / sampled step',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
