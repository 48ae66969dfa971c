"""
Rows per second of the exact noisy forward at n = 7..9 (qhea_model_forward_noisy_exact_wide: the density matrix tiled through
device memory) beside the trajectory call (qhea_model_forward_noisy_wide, T = 1000 trajectories) and the ideal forward
(qhea_model_forward_chunks), same rows, same run:
  (a) bench.py's cfg 4 model: HEAQNN Q8 20 x 2, 102 inputs, 10^4 rows;
  (b) QuanONet Q7 Net20-2-10-2, 10^4 rows;
  (c) QuanONet Q9 Net20-2-10-2, 1024 rows.
From these the cross-over T* = (time of the exact call) / (time of the trajectory call per trajectory): the trajectory count
above which the exact value is the cheaper one.  By byte count a stage reads and writes rho once, 2 * 4^n * 16 bytes per row, and
a sub-layer is two stages: 'bytes_per_row_estimate' and the bandwidth it implies are an ESTIMATE from that count, not a counter.
Then the chunk sweep at n = 8 and 9 (cases a and c): the density matrices of a chunk at 64 MiB, 256 MiB and 1 GiB, each timed
`--reps` times (the default chunk is WIDE_EXACT_STATE_BYTES of quanonet_amd/noise.py, recorded as 'default_state_bytes');
'spread' is (max - min) / median of one setting's own repetitions.
Times: CUDA events around one host call, 2 warm-up calls, median of `--reps`.
    python scripts/exact_noisy_wide_rate.py [--out profiles/r37_exact_noisy_wide_rate.json] [--only a|b|c] [--exact-only]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quanonet_amd import _lib                                                    # noqa: E402
from quanonet_amd import noise as noise_module                                  # noqa: E402
from quanonet_amd.noise import WIDE_EXACT_STATE_BYTES, NoiseModel, noisy_predict, wide_exact_noisy_predict     # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402
from scripts.noisy_traj_training_rate import _heaqnn                             # noqa: E402

CASES = {'a': ('a: HEAQNN Q8 20 x 2, 102 inputs, 1e4 rows', 'heaqnn', 8, (20, 2), 102, 10000),
         'b': ('b: QuanONet Q7 Net20-2-10-2, 1e4 rows', 'quanonet', 7, (20, 2, 10, 2), 100, 10000),
         'c': ('c: QuanONet Q9 Net20-2-10-2, 1024 rows', 'quanonet', 9, (20, 2, 10, 2), 100, 1024)}
TRAJECTORIES = 1000
SWEEP_STATE_BYTES = (1 << 26, 1 << 28, 1 << 30)


def _stat(t, rows):
    med, lo, hi = t
    return {'seconds_median': med, 'seconds_min': lo, 'seconds_max': hi, 'rows_per_s': rows / med, 'spread': (hi - lo) / med}


def case(key, reps, exact_only, dev):
    name, kind, n, net, b_in, rows = CASES[key]
    if kind == 'heaqnn':
        m, ins = _heaqnn(n, net, b_in, dev), (_inputs(rows, b_in, dev)[0],)
        sublayers = net[0] * net[1]
    else:
        m, ins = _model(n, net, b_in, dev), _inputs(rows, b_in, dev)
        sublayers = net[0] * net[1] + net[2] * net[3]
    noise = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2, trajectories=TRAJECTORIES, seed=7)
    out = {'case': name, 'rows': rows, 'noise': noise.asdict(), 'stage_launches': 2 * sublayers,
           'default_state_bytes': WIDE_EXACT_STATE_BYTES}
    out['exact'] = _stat(_time(lambda: wide_exact_noisy_predict(m, ins, noise), reps), rows)
    # the first stage loads nothing
    out['bytes_per_row_estimate'] = (2 * 2 * sublayers - 1) * 4 ** n * 16
    out['bandwidth_estimate_TB_per_s'] = out['bytes_per_row_estimate'] * rows / out['exact']['seconds_median'] * 1e-12
    if n >= 8:
        out['chunk_sweep'] = []
        for state in SWEEP_STATE_BYTES:
            chunk = state >> (2 * n + 4)
            noise_module.WIDE_EXACT_STATE_BYTES = state                  # chunk_rows alone only lowers the default
            st = _stat(_time(lambda: wide_exact_noisy_predict(m, ins, noise), reps), rows)
            noise_module.WIDE_EXACT_STATE_BYTES = WIDE_EXACT_STATE_BYTES
            out['chunk_sweep'].append(dict(st, state_bytes=state, chunk_rows=chunk))
    if exact_only:
        return out
    med = out['exact']['seconds_median']
    med_t, lo, hi = _time(lambda: noisy_predict(m, ins, noise, chunk_rows=rows), reps)
    out['trajectories'] = {'values_per_row': TRAJECTORIES, 'seconds_median': med_t, 'seconds_min': lo, 'seconds_max': hi,
                           'circuit_runs_per_s': rows * TRAJECTORIES / med_t}
    desc, flat = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    med_i, lo, hi = _time(lambda: _lib.model_forward_chunks(desc, ins[0], ins[1] if len(ins) > 1 else None, flat, 16384), reps)
    out['ideal'] = {'seconds_median': med_i, 'seconds_min': lo, 'seconds_max': hi, 'evaluations_per_s': rows / med_i}
    out['crossover_trajectories'] = med / (med_t / TRAJECTORIES)
    out['exact_over_ideal'] = med / med_i
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r37_exact_noisy_wide_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--exact-only', action='store_true', help='time the exact call alone (profiling runs)')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.reps, args.exact_only, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None and not args.exact_only:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': 'CUDA events around one host call, 2 warm-up calls, median of '
                         f'{args.reps}; exact = wide_exact_noisy_predict at its default chunk (prep + value tables + stages + '
                         f'read-out per chunk); trajectories = prep + trajectory kernel + finish at T = {TRAJECTORIES}; ideal = '
                         'qhea_model_forward_chunks; crossover_trajectories = exact seconds / (trajectory seconds / T); '
                         'bytes_per_row_estimate = (2 * stages - 1) * 4^n * 16, an estimate by byte count; chunk_sweep: the '
                         'density matrices of a chunk at 64 MiB, 256 MiB, 1 GiB, spread = (max - min) / median of the '
                         'repetitions of one setting',
               'results': res}
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
