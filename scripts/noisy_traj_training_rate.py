"""
Time per training step of sampled-trajectory noise-aware training (qhea_model_train_steps_noisy_wide, n = 7..9) beside, on the
same rows and in the same run, the ideal training step (qhea_model_train_steps) and the sampled forward
(qhea_model_forward_noisy_wide, rows x T trajectories):
  (a) HEAQNN Q8 20 x 2, 102 inputs, batch 100 (bench.py's cfg 4 model at the paper's batch);   (b) the same, batch 2048 (cfg 4);
  (c) QuanONet Q7 Net20-2-10-2, batch 100;   (d) QuanONet Q9 Net20-2-10-2, batch 100.
T = 16, 64, 256.  Noise: p1 = 1e-3, p2 = 1e-2, readout = 1e-2.  Times: device events around ONE train_steps call of `--steps`
steps (the forward: around `--steps` calls), 2 warm-up calls, median of `--reps`; reported per step, per trajectory, and as the
ratio of the step's time per trajectory to the forward call's.
    python scripts/noisy_traj_training_rate.py [--out profiles/r29_noisy_traj_training_rate.json] [--only a|b|c|d] [--T 64]
                                               [--grad-only]
(--grad-only times the new call alone: profiling runs, and runs of a library built with another QHEA_NOISE_GRAD_TILE through
the QHEA_LIB environment variable.)
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
from quanonet_amd.models import HEAQNNPT                                         # noqa: E402
from quanonet_amd.noise import NoiseModel                                        # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402

CASES = {'a': ('a: HEAQNN Q8 20 x 2, 102 inputs, batch 100', 'heaqnn', 8, (20, 2), 102, 100),
         'b': ('b: HEAQNN Q8 20 x 2, 102 inputs, batch 2048', 'heaqnn', 8, (20, 2), 102, 2048),
         'c': ('c: QuanONet Q7 Net20-2-10-2, batch 100', 'quanonet', 7, (20, 2, 10, 2), 100, 100),
         'd': ('d: QuanONet Q9 Net20-2-10-2, batch 100', 'quanonet', 9, (20, 2, 10, 2), 100, 100)}
TS = (16, 64, 256)


def _heaqnn(n, net, x_in, dev, seed=0):
    torch.manual_seed(seed)
    m = HEAQNNPT(n, x_in, net, scale_coeff=0.1, if_trainable_freq=True).double().to(dev)
    with torch.no_grad():
        for p in m.parameters():
            p.uniform_(-1.0, 1.0)
    return m


def _stat(t, steps):
    med, lo, hi = t
    return {'seconds_median': med / steps, 'seconds_min': lo / steps, 'seconds_max': hi / steps}


def case(key, Ts, steps, reps, grad_only, dev):
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
    res = {'case': name, 'batch': batch, 'steps_per_call': steps, 'parameters': P, 'library': os.path.relpath(_lib.LIB_PATH, ROOT)}

    def state():
        return flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0)

    if not grad_only:
        p2, m2, v2 = state()
        ideal = lambda: _lib.model_train_steps(desc, bounds, sizes, ins[0], ins[1], y, p2, out, m2, v2, 1, 1e-4, 0.9, 0.999, 1e-8,
                                               0.0)
        t_ideal = _time(ideal, reps)
        res['ideal_step'] = _stat(t_ideal, steps)
    res['by_T'] = []
    pred = torch.empty(batch, dtype=torch.float64, device=dev)
    for T in Ts:
        noise = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2, trajectories=T, seed=7)
        nz = noise.params()
        p, mm, vv = state()
        grad = lambda: _lib.model_train_steps_noisy_wide(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-4, 0.9,
                                                         0.999, 1e-8, 0.0, nz)
        t_grad = _time(grad, reps)
        r = {'T': T, 'noise': noise.asdict(), 'noisy_step': _stat(t_grad, steps),
             'noisy_step_seconds_per_trajectory': t_grad[0] / steps / (batch * T)}
        if not grad_only:
            def forward():
                for i in range(steps):
                    a, b = bounds[i], bounds[i + 1]
                    _lib.model_forward_noisy_wide(desc, ins[0][a:b], None if ins[1] is None else ins[1][a:b], flat0, nz, row0=a,
                                                  out=pred)
            t_fwd = _time(forward, reps)
            r['sampled_forward'] = _stat(t_fwd, steps)
            r['sampled_forward_seconds_per_trajectory'] = t_fwd[0] / steps / (batch * T)
            r['step_over_forward_per_trajectory'] = t_grad[0] / t_fwd[0]
            r['step_over_ideal_step'] = t_grad[0] / t_ideal[0]
        res['by_T'].append(r)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r29_noisy_traj_training_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--T', type=int, default=None, help='one trajectory count instead of 16, 64, 256')
    ap.add_argument('--grad-only', action='store_true', help='time the new call alone (profiling and tile runs)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, TS if args.T is None else (args.T,), args.steps, args.reps, args.grad_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and args.T is None and not args.grad_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call of {args.steps} steps (sampled forward: {args.steps} calls), 2 '
                         f'warm-up calls, median of {args.reps}, per step; noisy step = prep + trajectory kernel (forward walk, '
                         'two reverse walks, inner products) + fold + reduce/Adam; sampled forward = prep + trajectory kernel + '
                         'finish on the same rows x T; ideal step = qhea_model_train_steps',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
