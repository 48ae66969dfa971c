"""
Time per training step of quantum-jump training under a device noise model at n = 10..12
(qhea_model_train_steps_noisy_device_lds) beside, on the same rows and in the same run, the quantum-jump forward
(qhea_model_forward_noisy_device_wide, rows x T trajectories) and the sampled-trajectory training step under uniform gate noise
(qhea_model_train_steps_noisy_lds):
  (a) QuanONet Q10 Net20-2-10-2, batch 100, T = 16 and 64;
  (b) the cfg 5 model QuanONet Q12 Net40-2-20-2, batch 100, T = 16;   (c) the same at its shard of 1024, T = 16.
Device setting: that of scripts/device_traj_wide_rate.py (every wire different), idle decay on; uniform rates p1 = 1e-3,
p2 = 1e-2, readout = 1e-2.  Times: device events around ONE train_steps call of a few steps (the forward: around as many calls),
2 warm-up calls, median of `--reps`; reported per step, per trajectory, and as the ratio of the step's time per trajectory to the
forward call's.  Also: the mean number of fired jumps per trajectory (numpy replay of 2 rows x 4 trajectories,
tests/device_traj_grad_reference.py) and the workspace of the call.
    python scripts/device_traj_lds_training_rate.py [--out profiles/r32_device_traj_lds_training_rate.json] [--only a|b|c]
                                                    [--grad-only] [--reps 5]
(--grad-only times the new call alone: runs of a library built with another QHEA_DEVICE_GRAD_LDS_TILE, or with
QHEA_DEVICE_GRAD_SKIP_REWALK for the share of the re-walks, through the QHEA_LIB environment variable.)
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quanonet_amd import _lib                                                    # noqa: E402
from quanonet_amd.noise import NoiseModel, Sampling                              # noqa: E402
from scripts.device_noise_rate import device_noise                               # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402
from scripts.noisy_traj_training_rate import _stat                               # noqa: E402

# name, n, net, inputs, batch, steps per call, trajectory counts
CASES = {'a': ('a: QuanONet Q10 Net20-2-10-2, batch 100', 10, (20, 2, 10, 2), 100, 100, 5, (16, 64)),
         'b': ('b: QuanONet Q12 Net40-2-20-2 (cfg 5), batch 100', 12, (40, 2, 20, 2), 100, 100, 3, (16,)),
         'c': ('c: QuanONet Q12 Net40-2-20-2 (cfg 5), batch 1024', 12, (40, 2, 20, 2), 100, 1024, 2, (16,))}


def mean_jumps(m, ins, dn, n):
    """fired jumps per trajectory of the first 2 rows x 4 trajectories, from the numpy replay"""
    from tests import device_traj_grad_reference as G
    from tests.test_noisy_forward import _circuit
    cpu = tuple(t[:2].cpu() for t in ins)
    c, _ = _circuit(m.cpu(), cpu)
    d = {k: [dn._at(k, q) for q in range(n)] for k in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2')}
    d.update(t_rx=dn.t_rx, t_rot=dn.t_rot, t_cx=dn.t_cx, idle=dn.idle)
    r = G.walk(c['n'], c['cfgs'], c['x'], c['w'], d, 4, 7, c['offset'], c['coeff'], c['ham_diag'], c['ham_pauli'], grad=False)
    return float(G.coverage(r, n, 4)['jumps'].mean())


def case(key, reps, grad_only, dev):
    name, n, net, b_in, batch, steps, Ts = CASES[key]
    rows = steps * batch
    m = _model(n, net, b_in, dev)
    ins = _inputs(rows, b_in, dev)
    y = torch.tensor(np.random.default_rng(2).normal(scale=0.5, size=rows), device=dev)
    desc, flat0 = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    P = flat0.numel()
    bounds, sizes = [i * batch for i in range(steps + 1)], [batch] * steps
    out = torch.zeros(steps, P + 2, dtype=torch.float64, device=dev)
    dn = dataclasses.replace(device_noise(n), idle=True)
    rec = dn.params(n)
    res = {'case': name, 'batch': batch, 'steps_per_call': steps, 'parameters': P, 'library': os.path.relpath(_lib.LIB_PATH, ROOT),
           'noise': dn.asdict(), 'by_T': []}

    def state():
        return flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0)

    pred = torch.empty(batch, dtype=torch.float64, device=dev)
    for T in Ts:
        sp = Sampling(trajectories=T, seed=7).params()
        p, mm, vv = state()
        grad = lambda: _lib.model_train_steps_noisy_device_lds(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-4, 0.9,
                                                               0.999, 1e-8, 0.0, rec, sp)
        t_grad = _time(grad, reps)
        r = {'T': T, 'device_step': _stat(t_grad, steps), 'device_step_seconds_per_trajectory': t_grad[0] / steps / (batch * T),
             'workspace_bytes': _lib.model_noisy_device_lds_grad_workspace_bytes(desc, batch, sp)}
        if not grad_only:
            def forward():
                for i in range(steps):
                    a, b = bounds[i], bounds[i + 1]
                    _lib.model_forward_noisy_device_wide(desc, ins[0][a:b], ins[1][a:b], flat0, rec, sp, row0=a, out=pred)
            t_fwd = _time(forward, reps)
            r['device_forward'] = _stat(t_fwd, steps)
            r['device_forward_seconds_per_trajectory'] = t_fwd[0] / steps / (batch * T)
            r['step_over_forward_per_trajectory'] = t_grad[0] / t_fwd[0]
            nz = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2, trajectories=T, seed=7).params()
            p2, m2, v2 = state()
            uniform = lambda: _lib.model_train_steps_noisy_lds(desc, bounds, sizes, ins[0], ins[1], y, p2, out, m2, v2, 1, 1e-4,
                                                               0.9, 0.999, 1e-8, 0.0, nz)
            t_uni = _time(uniform, reps)
            r['uniform_step'] = _stat(t_uni, steps)
            r['device_step_over_uniform_step'] = t_grad[0] / t_uni[0]
        res['by_T'].append(r)
    if not grad_only:
        res['mean_fired_jumps_per_trajectory'] = mean_jumps(m, ins, dn, n)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r32_device_traj_lds_training_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--grad-only', action='store_true', help='time the new call alone (tile and re-walk runs)')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.reps, args.grad_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and not args.grad_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call of steps_per_call steps (device forward: as many calls), 2 warm-up '
                         f'calls, median of {args.reps}, per step; device step = tables + prep + trajectory kernel (forward walk with '
                         'snapshots and words, two reverse walks, inner products, at most one block re-walked per fired jump) + fold '
                         '+ reduce/Adam; device forward = prep + tables + trajectory kernel + finish on the same rows x T; uniform '
                         'step = qhea_model_train_steps_noisy_lds under p1 = 1e-3, p2 = 1e-2, readout = 1e-2',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
