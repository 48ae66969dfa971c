"""
Time per training step under a device noise model with rho replayed from stored states
(qhea_model_train_steps_noisy_device_exact_stored):
  (a) inside the inverse walk's bound, beside the inverse step (qhea_model_train_steps_noisy_device_exact) on the same rows in
      the same run, and their ratio: Q5 Net20-2-10-2 at batch 100 and 1000, Q6 Net20-2-10-2 at batch 100;
  (b) past it, stored only, with the workspace: Q5 Net40-2-20-2 (the headline model, log10 A_dev 10.99) at batch 100 and 1000.
The device setting is scripts/device_noise_rate.py's (every wire different, idle decay on).  Times: device events around ONE
train_steps call of `--steps` steps, 2 warm-up calls, median of `--reps`; reported per step.  Beside every stored step stands
the byte count of its snapshots (written once and read once per step) and the HBM time that count alone would take at
`--hbm-tbs` TB/s -- an ESTIMATE from the byte count, not a measurement.
    python scripts/device_noise_stored_rate.py [--out profiles/r33_device_noise_stored_rate.json] [--only a1|a2|a3|b1|b2]
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

from quanonet_amd import _lib                                                            # noqa: E402
from quanonet_amd.noise import device_amplification, device_layer_amplification          # noqa: E402
from scripts.device_noise_rate import device_noise                                       # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                               # noqa: E402

CASES = {'a1': ('a: Q5 Net20-2-10-2, batch 100', 5, (20, 2, 10, 2), 100, 100, True),
         'a2': ('a: Q5 Net20-2-10-2, batch 1000', 5, (20, 2, 10, 2), 100, 1000, True),
         'a3': ('a: Q6 Net20-2-10-2, batch 100', 6, (20, 2, 10, 2), 100, 100, True),
         'b1': ('b: Q5 Net40-2-20-2, batch 100', 5, (40, 2, 20, 2), 100, 100, False),
         'b2': ('b: Q5 Net40-2-20-2, batch 1000', 5, (40, 2, 20, 2), 100, 1000, False)}


def _stat(t, steps):
    med, lo, hi = t
    return {'seconds_median': med / steps, 'seconds_min': lo / steps, 'seconds_max': hi / steps}


def case(key, steps, reps, hbm_tbs, dev):
    name, n, net, b_in, batch, with_inverse = CASES[key]
    m = _model(n, net, b_in, dev)
    rows = steps * batch
    ins = _inputs(rows, b_in, dev)
    y = torch.tensor(np.random.default_rng(2).normal(scale=0.5, size=rows), device=dev)
    dn = device_noise(n)
    desc, flat0 = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    P = flat0.numel()
    bounds, sizes = [i * batch for i in range(steps + 1)], [batch] * steps
    out = torch.zeros(steps, P + 2, dtype=torch.float64, device=dev)
    rec = dn.params(n)
    ws_stored = _lib.model_device_noisy_stored_grad_workspace_bytes(desc, batch)
    snap = _lib.model_device_noisy_stored_grad_workspace_bytes(desc, batch, snapshots_only=True)
    res = {'case': name, 'batch': batch, 'steps_per_call': steps, 'parameters': P, 'noise': dn.asdict(),
           'log10_amplification': device_amplification(m, dn), 'log10_layer_amplification': device_layer_amplification(m, dn),
           'workspace_bytes_stored': ws_stored, 'snapshot_bytes': snap,
           'estimate_from_byte_count': {'bytes_moved_per_step': 2 * snap, 'assumed_hbm_TB_per_s': hbm_tbs,
                                        'seconds_per_step': 2 * snap / (hbm_tbs * 1e12),
                                        'note': 'an estimate: snapshot bytes written once and read once at the assumed rate'}}

    def timed(call):
        p, mm, vv = flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0)
        return _time(lambda: call(desc, bounds, sizes, ins[0], ins[1], y, p, out, mm, vv, 1, 1e-4, 0.9, 0.999, 1e-8, 0.0, rec), reps)

    stored = timed(_lib.model_train_steps_noisy_device_exact_stored)
    res['stored_step'] = _stat(stored, steps)
    if with_inverse:
        inverse = timed(_lib.model_train_steps_noisy_device_exact)
        again = timed(_lib.model_train_steps_noisy_device_exact_stored)       # the stored step once more, behind the inverse one
        res['inverse_step'] = _stat(inverse, steps)
        res['stored_step_again'] = _stat(again, steps)
        res['stored_over_inverse'] = stored[0] / inverse[0]
        res['stored_again_over_inverse'] = again[0] / inverse[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r33_device_noise_stored_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--hbm-tbs', type=float, default=4.0, help='HBM rate assumed by the byte-count estimate, TB/s')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.steps, args.reps, args.hbm_tbs, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call of {args.steps} steps, 2 warm-up calls, median of {args.reps}, per '
                         'step; stored step = (table kernel once per call) + prep + density_dev_stored_bwd_kernel + reduce/Adam, '
                         'inverse step = the same with density_dev_bwd_kernel, both under the DeviceNoise of '
                         'scripts/device_noise_rate.py on the same rows; (b) is past the inverse walk\'s bound and has no inverse '
                         'step; estimate_from_byte_count is arithmetic on the snapshot size, not a measurement',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
