"""
Rows per second of the exact forward under a device noise model at n = 7..9 (qhea_model_forward_noisy_device_exact_wide) beside,
in the same run and on the same rows,
  * the uniform tiled call (wide_exact_noisy_predict) on the same model with DeviceNoise.uniform's rates as a NoiseModel,
  * the quantum-jump call (device_noisy_predict, T = 1000 trajectories, expectation mode),
  * the ideal forward (qhea_model_forward_chunks),
on the three workloads of scripts/exact_noisy_wide_rate.py:
  (a) bench.py's cfg 4 model: HEAQNN Q8 20 x 2, 102 inputs, 10^4 rows;
  (b) QuanONet Q7 Net20-2-10-2, 10^4 rows;
  (c) QuanONet Q9 Net20-2-10-2, 1024 rows.
The device setting is the uniform rates on every wire and slot plus relaxation with the ring's idle decay (T1 = 100, T2 = 80,
t_rx = t_rot = 0.05, t_cx = 0.3 in one unit): every site of every wire is a channel other than the identity, which is what the
kernels cost in any setting -- the sites are applied whatever their values.
Reported: 'ratio_to_uniform' (this call's time over the uniform tiled call's), 'crossover_trajectories' T* = (time of the exact
call) / (time of the quantum-jump call per trajectory), and 'bandwidth_estimate_TB_per_s' from 'bytes_per_row_estimate' =
(2 x stages - 1) x 4^n x 16: an ESTIMATE by byte count (a stage reads and writes rho once, the first stage loads nothing),
not a counter.
Times: device events around one host call, 2 warm-up calls, median of `--reps` (5).
    python scripts/device_exact_noisy_wide_rate.py [--out profiles/r39_device_exact_noisy_wide_rate.json] [--only a|b|c]
--jump-probe: the quantum-jump call alone (median of 3) on the models of (a) and (b) and on both at half their depth, at
(T, rows) = (1000, 10^4), (500, 10^4), (1000, 5000), (250, 10^4) -> profiles/r39_jump_time_probe.json.  It answers why the
quantum-jump times of (a) and (b) agree: the time is proportional to T x rows and to the depth (no constant cost, no effect of
the chunking), and a sub-layer at n = 8 costs 1.50 times a sub-layer at n = 7 while (b) has 60 sub-layers against (a)'s 40.
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
from quanonet_amd.noise import (WIDE_EXACT_STATE_BYTES, DeviceNoise, NoiseModel, Sampling, device_exact_noisy_predict,    # noqa: E402
                                device_noisy_predict, wide_exact_noisy_predict)
from scripts.exact_noisy_wide_rate import CASES, TRAJECTORIES, _stat            # noqa: E402
from scripts.noisy_eval_rate import _inputs, _model, _time                       # noqa: E402
from scripts.noisy_traj_training_rate import _heaqnn                             # noqa: E402

RELAXATION = dict(t1=100.0, t2=80.0, t_rx=0.05, t_rot=0.05, t_cx=0.3, idle=True)


def case(key, reps, dev):
    name, kind, n, net, b_in, rows = CASES[key]
    if kind == 'heaqnn':
        m, ins = _heaqnn(n, net, b_in, dev), (_inputs(rows, b_in, dev)[0],)
        sublayers = net[0] * net[1]
    else:
        m, ins = _model(n, net, b_in, dev), _inputs(rows, b_in, dev)
        sublayers = net[0] * net[1] + net[2] * net[3]
    nm = NoiseModel(p1=1e-3, p2=1e-2, readout=1e-2)
    dn = DeviceNoise(p1=nm.p1, p2=nm.p2, readout01=nm.readout, readout10=nm.readout, **RELAXATION)
    sampling = Sampling(trajectories=TRAJECTORIES, seed=7)
    out = {'case': name, 'rows': rows, 'device_noise': dn.asdict(), 'uniform_noise': nm.asdict(), 'stage_launches': 2 * sublayers,
           'default_state_bytes': WIDE_EXACT_STATE_BYTES}
    out['device_exact'] = _stat(_time(lambda: device_exact_noisy_predict(m, ins, dn), reps), rows)
    out['uniform_exact'] = _stat(_time(lambda: wide_exact_noisy_predict(m, ins, nm), reps), rows)
    med, med_u = out['device_exact']['seconds_median'], out['uniform_exact']['seconds_median']
    out['ratio_to_uniform'] = med / med_u
    out['bytes_per_row_estimate'] = (2 * 2 * sublayers - 1) * 4 ** n * 16
    out['bandwidth_estimate_TB_per_s'] = out['bytes_per_row_estimate'] * rows / med * 1e-12
    med_t, lo, hi = _time(lambda: device_noisy_predict(m, ins, dn, sampling, chunk_rows=rows), reps)
    out['quantum_jump'] = {'values_per_row': TRAJECTORIES, 'seconds_median': med_t, 'seconds_min': lo, 'seconds_max': hi,
                           'circuit_runs_per_s': rows * TRAJECTORIES / med_t}
    desc, flat = m.fused_desc(), torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    med_i, lo, hi = _time(lambda: _lib.model_forward_chunks(desc, ins[0], ins[1] if len(ins) > 1 else None, flat, 16384), reps)
    out['ideal'] = {'seconds_median': med_i, 'seconds_min': lo, 'seconds_max': hi, 'evaluations_per_s': rows / med_i}
    out['crossover_trajectories'] = med / (med_t / TRAJECTORIES)
    out['exact_over_ideal'] = med / med_i
    return out


def jump_probe(dev):
    dn = DeviceNoise(p1=1e-3, p2=1e-2, readout01=1e-2, readout10=1e-2, **RELAXATION)
    models = {'Q8 heaqnn 20x2': (_heaqnn(8, (20, 2), 102, dev), (_inputs(10000, 102, dev)[0],)),
              'Q7 Net20-2-10-2': (_model(7, (20, 2, 10, 2), 100, dev), _inputs(10000, 100, dev)),
              'Q7 Net10-2-5-2': (_model(7, (10, 2, 5, 2), 100, dev), _inputs(10000, 100, dev)),
              'Q8 heaqnn 10x2': (_heaqnn(8, (10, 2), 102, dev), (_inputs(10000, 102, dev)[0],))}
    res = []
    for tag, (m, ins) in models.items():
        for T, rows in ((1000, 10000), (500, 10000), (1000, 5000), (250, 10000)):
            part, sp = tuple(t[:rows] for t in ins), Sampling(trajectories=T, seed=7)
            med, lo, hi = _time(lambda: device_noisy_predict(m, part, dn, sp, chunk_rows=rows), 3)
            res.append(dict(case=tag, T=T, rows=rows, seconds=med, lo=lo, hi=hi, us_per_circuit=med / (T * rows) * 1e6))
            print(json.dumps(res[-1]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r39_device_exact_noisy_wide_rate.json'))
    ap.add_argument('--only', choices=sorted(CASES), default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--jump-probe', action='store_true', help='the quantum-jump call alone at several T, rows and depths')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    if args.jump_probe:
        out = {'device': torch.cuda.get_device_name(0),
               'method': 'scripts/device_exact_noisy_wide_rate.py --jump-probe: device events around one device_noisy_predict '
                         'call (chunk_rows = rows, expectation mode, seed 7, the device setting of the rate run), 2 warm-up '
                         'calls, median of 3; four models x (T, rows) = (1000, 1e4), (500, 1e4), (1000, 5000), (250, 1e4)',
               'results': jump_probe(dev)}
        with open(os.path.join(ROOT, 'profiles', 'r39_jump_time_probe.json'), 'w') as f:
            json.dump(out, f, indent=1)
        return
    res = []
    for key in sorted(CASES):
        if args.only in (None, key):
            res.append(case(key, args.reps, dev))
            print(json.dumps(res[-1]), flush=True)
    if args.only is None:
        out = {'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
               'method': f'device events around one host call, 2 warm-up calls, median of {args.reps}; device_exact = '
                         'device_exact_noisy_predict at its default chunk (prep + value tables + stages + read-out per chunk); '
                         'uniform_exact = wide_exact_noisy_predict on the same model and rows with the same p1, p2, readout; '
                         f'quantum_jump = device_noisy_predict at T = {TRAJECTORIES}, expectation mode; ideal = '
                         'qhea_model_forward_chunks; ratio_to_uniform = device_exact seconds / uniform_exact seconds; '
                         'crossover_trajectories = device_exact seconds / (quantum_jump seconds / T); bytes_per_row_estimate = '
                         '(2 * stages - 1) * 4^n * 16 and the bandwidth from it are an estimate by byte count, not a counter',
               'results': res}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
