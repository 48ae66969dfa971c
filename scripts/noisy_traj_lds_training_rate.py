"""
Time per training step of sampled-trajectory noise-aware training at n = 10..12 (qhea_model_train_steps_noisy_lds) beside, in
the same run, two reference measurements:
  1. the sampled forward (qhea_model_forward_noisy_wide) on the same rows x T trajectories;
  2. the ideal training step (qhea_model_train_steps) on rows x T SAMPLES of the same model -- the yardstick: it walks as many
     states forward and back as the new call does, without the unfolded RX layers, the frames, the draws and the record's
     read-add-store.
Workloads:
  (a) QuanONet Q10 Net20-2-10-2, batch 100;   (b) the cfg 5 model QuanONet Q12 Net40-2-20-2, batch 100;
  (c) the same at its shard of 1024 (3 steps per call there: a step is of the order of a second).
T = 16, 64.  Noise: p1 = 1e-3, p2 = 1e-2, readout = 1e-2.  Times: device events around ONE host call, 2 warm-up calls, median of
`--reps`; reported per step, per trajectory, and as the two ratios per trajectory (per sample).
    python scripts/noisy_traj_lds_training_rate.py [--out profiles/r30_noisy_traj_lds_training_rate.json] [--only a|b|c] [--T 64]
                                                   [--grad-only] [--reps 5]
(--grad-only times the new call alone: profiling runs, and runs of a library built with another QHEA_NOISE_GRAD_LDS_TILE
through the QHEA_LIB environment variable.)
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
from scripts.noisy_traj_training_rate import _stat                               # noqa: E402

CASES = {'a': ('a: QuanONet Q10 Net20-2-10-2, batch 100', 10, (20, 2, 10, 2), 100, 100, 10),
         'b': ('b: QuanONet Q12 Net40-2-20-2 (cfg 5), batch 100', 12, (40, 2, 20, 2), 100, 100, 5),
         'c': ('c: QuanONet Q12 Net40-2-20-2 (cfg 5), batch 1024', 12, (40, 2, 20, 2), 100, 1024, 3)}
TS = (16, 64)


def case(key, Ts, reps, grad_only, dev):
    name, n, net, b_in, batch, steps = CASES[key]
    rows = steps * batch
    m = _model(n, net, b_in, dev)
    ins = _inputs(rows, b_in, dev)
    y = torch.tensor(np.random.default_rng(2).normal(scale=0.5, size=rows), device=dev)
    desc, flat0 = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    P = flat0.numel()
    bounds, sizes = [i * batch for i in range(steps + 1)], [batch] * steps
    out = torch.zeros(steps, P + 2, dtype=torch.float64, device=dev)
    res = {'case': name, 'batch': batch, 'steps_per_call': steps, 'parameters': P, 'library': os.path.relpath(_lib.LIB_PATH, ROOT),
           'by_T': []}

    def state():
        return flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0)

    pred = torch.empty(batch, dtype=torch.float64, device=dev)
    for T in Ts:
        noise = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2, trajectories=T, seed=7)
        nz = noise.params()
        p, mm, vv = state()
        grad = lambda: _lib.model_train_steps_noisy_lds(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-4, 0.9,
                                                        0.999, 1e-8, 0.0, nz)
        t_grad = _time(grad, reps)
        r = {'T': T, 'noise': noise.asdict(), 'noisy_step': _stat(t_grad, steps),
             'noisy_step_seconds_per_trajectory': t_grad[0] / steps / (batch * T),
             'workspace_bytes': _lib.model_noisy_lds_grad_workspace_bytes(desc, batch, nz)}
        if not grad_only:
            def forward():
                for i in range(steps):
                    a, b = bounds[i], bounds[i + 1]
                    _lib.model_forward_noisy_wide(desc, ins[0][a:b], ins[1][a:b], flat0, nz, row0=a, out=pred)
            t_fwd = _time(forward, reps)
            r['sampled_forward'] = _stat(t_fwd, steps)
            r['sampled_forward_seconds_per_trajectory'] = t_fwd[0] / steps / (batch * T)
            r['step_over_forward_per_trajectory'] = t_grad[0] / t_fwd[0]
            # the ideal step on batch x T samples (the step's rows, each T times): one step per call
            big = tuple(t[:batch].repeat(T, 1) for t in ins)
            yb = y[:batch].repeat(T)
            p2, m2, v2 = state()
            row = torch.zeros(1, P + 2, dtype=torch.float64, device=dev)
            ideal = lambda: _lib.model_train_steps(desc, [0, batch * T], [batch * T], big[0], big[1], yb, p2, row, m2, v2, 1, 1e-4,
                                                   0.9, 0.999, 1e-8, 0.0)
            t_ideal = _time(ideal, reps)
            r['ideal_step_on_rows_x_T_samples'] = _stat(t_ideal, 1)
            r['ideal_step_seconds_per_sample'] = t_ideal[0] / (batch * T)
            r['step_over_ideal_per_sample'] = (t_grad[0] / steps) / t_ideal[0]
            del big, yb
        res['by_T'].append(r)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r30_noisy_traj_lds_training_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--T', type=int, default=None, help='one trajectory count instead of 16, 64')
    ap.add_argument('--grad-only', action='store_true', help='time the new call alone (profiling and tile runs)')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, TS if args.T is None else (args.T,), args.reps, args.grad_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and args.T is None and not args.grad_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call (steps_per_call steps; sampled forward: as many calls; ideal step: '
                         f'one step of batch x T samples), 2 warm-up calls, median of {args.reps}; noisy step = prep + trajectory '
                         'kernel (forward walk, two reverse walks, inner products) + fold + reduce/Adam; sampled forward = prep + '
                         'trajectory kernel + finish on the same rows x T; ideal step = qhea_model_train_steps',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
