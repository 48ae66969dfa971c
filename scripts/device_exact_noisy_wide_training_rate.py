"""
Time per training step of exact device-noise training at n = 7..9 (qhea_model_train_steps_noisy_device_exact_wide: rho and O
tiled through device memory, the channel sites of a DeviceNoise) beside, on the same rows and in the same run,
  the uniform tiled step (qhea_model_train_steps_noisy_exact_wide, the NoiseModel with the same p1, p2 and readout),
  the device forward it is built on (qhea_model_forward_noisy_device_exact_wide), and
  the quantum-jump step (qhea_model_train_steps_noisy_device at T = 64).
Workloads:
  (b) HEAQNN Q8 20 x 2, 102 inputs, batch 100 (bench.py's cfg 4 model);   (c) the same, batch 2048 (cfg 4);
  (a) QuanONet Q7 Net20-2-10-2, batch 100;                                 (d) QuanONet Q9 Net20-2-10-2, batch 64.
Setting: that of scripts/device_exact_noisy_wide_rate.py (p1 = 1e-3, p2 = 1e-2, readout 1e-2, T1 = 100, T2 = 80, t_rx = t_rot =
0.05, t_cx = 0.3, idle on).  The inverse walk admits log10 A_dev <= 7: cfg 4 has 6.07 and runs as it is; the two 60-sub-layer
models have 7.28 and 11.12 and are refused, so (a) and (d) run with the three durations x 0.25 (3.56 and 5.02).  The factor and
log10 A_dev are recorded per row.
Times: device events around ONE train_steps call of `--steps` steps (the forward: around `--steps` calls), 2 warm-up calls,
median of `--reps` with min and max; reported per step.  T* is the trajectory count at which the quantum-jump step costs what
the exact step costs.
What the figures are set beside, stated before the run: the reverse stages do the uniform stages' memory traffic and LDS passes
with 10 more multiply-adds per element and site and 80 (ring pass) scalar table loads per pass, so the step should cost
1.05 .. 1.25 x the uniform step (n <= 6 measured 1.16 .. 1.20, the tiled forward 1.05 .. 1.06) and 4 .. 5 x the device forward
(the uniform step measured 3.9 .. 4.6 x its forward).  A ratio to the uniform step above 1.5 would want its cause found.
    python scripts/device_exact_noisy_wide_training_rate.py [--out profiles/r41_device_exact_noisy_wide_training_rate.json]
                                                            [--only a|b|c|d] [--exact-only]
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
from quanonet_amd.noise import DeviceNoise, NoiseModel, Sampling                 # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402
from scripts.noisy_traj_training_rate import _heaqnn, _stat                      # noqa: E402

# name, kind, n, net, inputs, batch, factor on the three durations
CASES = {'a': ('a: QuanONet Q7 Net20-2-10-2, batch 100', 'quanonet', 7, (20, 2, 10, 2), 100, 100, 0.25),
         'b': ('b: HEAQNN Q8 20 x 2, 102 inputs, batch 100', 'heaqnn', 8, (20, 2), 102, 100, 1.0),
         'c': ('c: HEAQNN Q8 20 x 2, 102 inputs, batch 2048', 'heaqnn', 8, (20, 2), 102, 2048, 1.0),
         'd': ('d: QuanONet Q9 Net20-2-10-2, batch 64', 'quanonet', 9, (20, 2, 10, 2), 100, 64, 0.25)}
T_JUMP = 64
RATES = dict(p1=1e-3, p2=1e-2, readout=1e-2)
RELAXATION = dict(t1=100.0, t2=80.0, t_rx=0.05, t_rot=0.05, t_cx=0.3)
EXPECTED = {'step_over_uniform_step': '1.05 .. 1.25', 'step_over_forward': '4 .. 5'}


def setting(factor):
    relax = dict(RELAXATION, **{k: factor * RELAXATION[k] for k in ('t_rx', 't_rot', 't_cx')})
    return DeviceNoise(p1=RATES['p1'], p2=RATES['p2'], readout01=RATES['readout'], readout10=RATES['readout'], idle=True, **relax)


def case(key, steps, reps, exact_only, dev):
    name, kind, n, net, b_in, batch, factor = CASES[key]
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
    dn, nm = setting(factor), NoiseModel(**RATES)
    rec, nz = dn.params(n), nm.params()
    res = {'case': name, 'batch': batch, 'steps_per_call': steps, 'parameters': P, 'device_noise': dn.asdict(),
           'duration_factor': factor, 'log10_A_dev': _lib.model_device_noisy_log10_amplification(desc, rec),
           'log10_A_dev_unscaled': _lib.model_device_noisy_log10_amplification(desc, setting(1.0).params(n)),
           'unscaled_refused': bool(_lib.model_device_noisy_wide_refused(desc, setting(1.0).params(n))),
           'workspace_bytes': _lib.model_device_noisy_wide_grad_workspace_bytes(desc, batch),
           'library': os.path.relpath(_lib.LIB_PATH, ROOT)}

    def state():
        return flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0)

    p, mm, vv = state()
    exact = lambda: _lib.model_train_steps_noisy_device_exact_wide(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-4,
                                                                   0.9, 0.999, 1e-8, 0.0, rec)
    t_exact = _time(exact, reps)
    res['device_exact_step'] = _stat(t_exact, steps)
    if exact_only:
        return res
    p1, m1, v1 = state()
    uniform = lambda: _lib.model_train_steps_noisy_exact_wide(desc, bounds, sizes, ins[0], ins[1], y, p1, out, m1, v1, 1, 1e-4, 0.9,
                                                              0.999, 1e-8, 0.0, nz)
    t_uni = _time(uniform, reps)
    res['uniform_exact_step'] = _stat(t_uni, steps)
    res['step_over_uniform_step'] = t_exact[0] / t_uni[0]
    pred = torch.empty(batch, dtype=torch.float64, device=dev)

    def forward():
        for i in range(steps):
            a, b = bounds[i], bounds[i + 1]
            _lib.model_forward_noisy_device_exact_wide(desc, ins[0][a:b], None if ins[1] is None else ins[1][a:b], flat0, rec,
                                                       out=pred)
    t_fwd = _time(forward, reps)
    res['device_exact_forward'] = _stat(t_fwd, steps)
    res['step_over_forward'] = t_exact[0] / t_fwd[0]
    res['expected'] = EXPECTED
    p2, m2, v2 = state()
    sp = Sampling(trajectories=T_JUMP, seed=7).params()
    jump = lambda: _lib.model_train_steps_noisy_device(desc, bounds, sizes, ins[0], ins[1], y, p2, out, m2, v2, 1, 1e-4, 0.9, 0.999,
                                                       1e-8, 0.0, rec, sp)
    t_jump = _time(jump, reps)
    res['jump_step_T64'] = _stat(t_jump, steps)
    res['T_star'] = T_JUMP * t_exact[0] / t_jump[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r41_device_exact_noisy_wide_training_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--exact-only', action='store_true', help='time the new call alone (profiling runs)')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in ('b', 'c', 'a', 'd'):
        if args.only in (None, key):
            res.append(case(key, args.steps, args.reps, args.exact_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and not args.exact_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call of {args.steps} steps (forward: {args.steps} calls), 2 warm-up calls, '
                         f'median of {args.reps} with min and max, per step; all calls of a workload in one run on the same rows; '
                         'device exact step = table + per step prep + value table + forward stages + read-out + O_N + reverse '
                         'stages + fold + reduce/Adam; uniform exact step = qhea_model_train_steps_noisy_exact_wide under the same '
                         f'p1, p2, readout; jump step = qhea_model_train_steps_noisy_device at T = {T_JUMP}; T* = {T_JUMP} x device '
                         'exact step / jump step',
               'expected_before_the_run': EXPECTED, 'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
