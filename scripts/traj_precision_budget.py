#!/usr/bin/env python
"""
Records what the error-budget table of the trajectory gradient kernels measures (tests/traj_precision_cases.py; the sampled-
Pauli and the quantum-jump units): per case and quantity the kernel's error against the extended-precision walk, e_ref (the two
fp64 numpy evaluations' own error against it: adjoint walk and shift, or stored and inverse walk), their ratio, the budget and
max|q|, with the kernel that ran and a jump case's LEVEL.

    python scripts/traj_precision_budget.py [--out profiles/r36_traj_precision_budget.json]

Needs a GPU and the built libraries.  A case whose kernel name differs from the table's is recorded with its assertion's text.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402
import torch                                                # noqa: E402

from tests import traj_precision_cases as TP                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r36_traj_precision_budget.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    props = torch.cuda.get_device_properties(dev)
    rec = {'device': props.name, 'factor': TP.FACTOR, 'trajectories': TP.T, 'lowered': {k: list(v) for k, v in TP.LOWERED.items()},
           'cases': []}
    for case in TP.CASES:
        ref = TP.reference(case)
        entry = {'id': case.id, 'family': case.family, 'n': case.n, 'net': list(case.net), 'rows': case.rows, 'readout': case.readout,
                 'rates': list(case.rates) if case.family == 'sampled' else None, 'tau': case.tau, 'hot_wires': case.hot, 'polar': case.polar, 'planned_level': case.level,
                 'level': float(TP.pattern_walk(case)['level'].max()) if case.family == 'jump' else None, 'quantities': {}}
        try:
            got, kernel = TP.run_case(dev, case)
        except AssertionError as e:
            entry['kernel_assertion'] = str(e)[:400]
            rec['cases'].append(entry)
            print(case.id, 'KERNEL', entry['kernel_assertion'], flush=True)
            continue
        entry['kernel'] = kernel
        for q in TP.QUANTITIES:
            error, e_ref, budget = TP.measure(got, ref, q)
            entry['quantities'][q] = {'error': error, 'e_ref': e_ref, 'e_first_walk': ref.e_c[q], 'e_second_walk': ref.e_np[q],
                                      'ratio': error / max(e_ref, 1e-300), 'budget': budget,
                                      'max_abs': TP._maxabs(ref.ld[q][0]), 'finite': bool(np.isfinite(got[q]).all()),
                                      'within': bool(error <= budget)}
        rec['cases'].append(entry)
        print(case.id, ' '.join(f"{q}={v['error']:.1e}/{v['ratio']:.1f}{'' if v['within'] else '!'}"
                                for q, v in entry['quantities'].items()), flush=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print('->', args.out)


if __name__ == '__main__':
    main()
