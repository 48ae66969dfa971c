"""
Time per training step of exact device-noise training from stored states at n = 7..9
(qhea_model_train_steps_noisy_device_exact_wide_stored: the forward sweep leaves rho after every unit in device memory, the
reverse walk starts every unit from it) beside, on the same rows and in the same run,
  the inverse walk (qhea_model_train_steps_noisy_device_exact_wide) where its guard admits the setting, and
  the quantum-jump step (qhea_model_train_steps_noisy_device at T = 64).
Workloads, under the setting of scripts/device_exact_noisy_wide_rate.py (p1 = 1e-3, p2 = 1e-2, readout 1e-2, T1 = 100, T2 = 80,
t_rx = t_rot = 0.05, t_cx = 0.3, idle on) with a factor on the three durations:
  (b) HEAQNN Q8 20 x 2, 102 inputs, batch 100 (bench.py's cfg 4 model), x 1, log10 A_dev 6.07: both walks;
  (c) the same, batch 2048: both walks;
  (a) QuanONet Q7 Net20-2-10-2, batch 100, x 0.25 (3.56): both walks;      (A) the same x 1 (7.28): the stored walk only;
  (d) QuanONet Q9 Net20-2-10-2, batch 64, x 0.25 (5.02): both walks;       (D) the same x 1 (11.12): the stored walk only,
      15 GiB of snapshots.
(A) and (D) also train through PTSolver with train_device_noise_exact='stored' (two epochs of `--steps` batches on synthetic
data); the wall time per step, evaluations included, and the solver's log line with its workspace are recorded.
Times: device events around ONE train_steps call of `--steps` steps, 2 warm-up calls, median of `--reps` with min and max;
reported per step.  T* is the trajectory count at which the quantum-jump step costs what the stored step costs.
What the figures are set beside, stated before the run: by byte count a stored step moves what an inverse step moves (a forward
stage reads a row and writes a row wherever they lie; a reverse unit reads rho once from the snapshot instead of the running
buffer) less one rho store per unit, 1 of 12 row transfers of a sub-layer; the reverse stages are not bandwidth-bound alone, so
the step should cost 0.95 .. 1.02 x the inverse step.  The snapshots do not stay in the 256 MiB of last-level cache at any
batch here, and neither do rho and O of the inverse walk past a few rows, so no cache effect is expected either way.  A ratio
above 1.05 would want its cause found.
    python scripts/device_exact_noisy_wide_stored_training_rate.py [--out profiles/r42_device_exact_noisy_wide_stored_training_rate.json]
                                                                   [--only a|A|b|c|d|D] [--stored-only] [--no-solver]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quanonet_amd import _lib                                                    # noqa: E402
from quanonet_amd.noise import Sampling                                          # noqa: E402
from scripts.device_exact_noisy_wide_training_rate import setting                # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402
from scripts.noisy_traj_training_rate import _heaqnn, _stat                      # noqa: E402

# name, kind, n, net, inputs, batch, factor on the three durations
CASES = {'b': ('b: HEAQNN Q8 20 x 2, 102 inputs, batch 100', 'heaqnn', 8, (20, 2), 102, 100, 1.0),
         'c': ('c: HEAQNN Q8 20 x 2, 102 inputs, batch 2048', 'heaqnn', 8, (20, 2), 102, 2048, 1.0),
         'a': ('a: QuanONet Q7 Net20-2-10-2, batch 100, durations x 0.25', 'quanonet', 7, (20, 2, 10, 2), 100, 100, 0.25),
         'A': ('A: QuanONet Q7 Net20-2-10-2, batch 100, durations x 1', 'quanonet', 7, (20, 2, 10, 2), 100, 100, 1.0),
         'd': ('d: QuanONet Q9 Net20-2-10-2, batch 64, durations x 0.25', 'quanonet', 9, (20, 2, 10, 2), 100, 64, 0.25),
         'D': ('D: QuanONet Q9 Net20-2-10-2, batch 64, durations x 1', 'quanonet', 9, (20, 2, 10, 2), 100, 64, 1.0)}
T_JUMP = 64
EXPECTED = {'stored_step_over_inverse_step': '0.95 .. 1.02'}


def solver_run(n, net, b_in, batch, steps, dn, dev):
    """two epochs of `steps` batches through PTSolver with train_device_noise_exact='stored': (seconds per step, log line)"""
    from quanonet_amd.solver import PTSolver, set_random_seed
    rng = np.random.default_rng(3)

    def part(r):
        b, t = rng.uniform(-1, 1, (r, b_in)), rng.uniform(0, 1, (r, 1))
        return b, t, np.sin(t[:, :1] * b[:, :1])
    trb, trt, tro = part(steps * batch)
    teb, tet, teo = part(batch)
    data = {'train_branch_input': trb, 'train_trunk_input': trt, 'train_output': tro,
            'test_branch_input': teb, 'test_trunk_input': tet, 'test_output': teo}
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': n, 'net_size': list(net), 'scale_coeff': 0.1,
               'if_trainable_freq': 'true', 'learning_rate': 1e-4, 'batch_size': batch, 'num_epochs': 2, 'seed': 0,
               'prefix': os.path.join(tmp, 'run'), 'run_id': 'r0', 'eval_batch_size': batch, 'if_save': False,
               'train_device_noise': dn.asdict(), 'train_device_noise_exact': 'stored'}
        set_random_seed(0)
        s = PTSolver(cfg, data, device=dev, log=lambda *a, **k: lines.append(' '.join(map(str, a))))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hist = s.train()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    said = [ln for ln in lines if 'stored states' in ln]
    return {'epochs': 2, 'steps_per_epoch': steps, 'wall_seconds_per_step_with_evaluation': wall / (2 * steps),
            'loss_train': [float(v) for v in hist['loss_train']], 'log': said[0] if said else None}


def case(key, steps, reps, stored_only, solver, dev):
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
    dn = setting(factor)
    rec = dn.params(n)
    inverse_runs = not _lib.model_device_noisy_wide_refused(desc, rec)
    res = {'case': name, 'batch': batch, 'steps_per_call': steps, 'parameters': P, 'device_noise': dn.asdict(),
           'duration_factor': factor, 'log10_A_dev': _lib.model_device_noisy_log10_amplification(desc, rec),
           'log10_A_dev_layer': _lib.model_device_noisy_log10_layer_amplification(desc, rec),
           'inverse_walk_refused': not inverse_runs,
           'workspace_bytes': _lib.model_device_noisy_wide_stored_grad_workspace_bytes(desc, batch),
           'snapshot_bytes': _lib.model_device_noisy_wide_stored_grad_workspace_bytes(desc, batch, snapshots_only=True),
           'inverse_workspace_bytes': _lib.model_device_noisy_wide_grad_workspace_bytes(desc, batch),
           'library': os.path.relpath(_lib.LIB_PATH, ROOT)}

    def state():
        return flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0)

    p, mm, vv = state()
    stored = lambda: _lib.model_train_steps_noisy_device_exact_wide_stored(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1,
                                                                           1e-4, 0.9, 0.999, 1e-8, 0.0, rec)
    t_stored = _time(stored, reps)
    res['stored_step'] = _stat(t_stored, steps)
    if stored_only:
        return res
    if inverse_runs:
        p1, m1, v1 = state()
        inverse = lambda: _lib.model_train_steps_noisy_device_exact_wide(desc, bounds, sizes, ins[0], ins[1], y, p1, out, m1, v1, 1,
                                                                         1e-4, 0.9, 0.999, 1e-8, 0.0, rec)
        t_inv = _time(inverse, reps)
        res['inverse_step'] = _stat(t_inv, steps)
        res['stored_step_over_inverse_step'] = t_stored[0] / t_inv[0]
        res['expected'] = EXPECTED
    p2, m2, v2 = state()
    sp = Sampling(trajectories=T_JUMP, seed=7).params()
    jump = lambda: _lib.model_train_steps_noisy_device(desc, bounds, sizes, ins[0], ins[1], y, p2, out, m2, v2, 1, 1e-4, 0.9, 0.999,
                                                       1e-8, 0.0, rec, sp)
    t_jump = _time(jump, reps)
    res['jump_step_T64'] = _stat(t_jump, steps)
    res['T_star'] = T_JUMP * t_stored[0] / t_jump[0]
    if solver and not inverse_runs and kind == 'quanonet':
        del out, p, mm, vv, p2, m2, v2
        res['ptsolver'] = solver_run(n, net, b_in, batch, steps, dn, dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r42_device_exact_noisy_wide_stored_training_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--stored-only', action='store_true', help='time the new call alone (profiling runs)')
    ap.add_argument('--no-solver', action='store_true', help='skip the PTSolver runs of (A) and (D)')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in ('b', 'c', 'a', 'A', 'd', 'D'):
        if args.only in (None, key):
            res.append(case(key, args.steps, args.reps, args.stored_only, not args.no_solver, dev))
            print(json.dumps(res[-1]), flush=True)
            torch.cuda.empty_cache()
    if args.only is None and not args.stored_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call of {args.steps} steps, 2 warm-up calls, median of {args.reps} with '
                         'min and max, per step; all calls of a workload in one run on the same rows; stored step = '
                         'qhea_model_train_steps_noisy_device_exact_wide_stored, inverse step = '
                         'qhea_model_train_steps_noisy_device_exact_wide (where its guard admits the setting); jump step = '
                         f'qhea_model_train_steps_noisy_device at T = {T_JUMP}; T* = {T_JUMP} x stored step / jump step; ptsolver = '
                         "two epochs through PTSolver with train_device_noise_exact='stored', wall time with its evaluations",
               'expected_before_the_run': EXPECTED, 'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
