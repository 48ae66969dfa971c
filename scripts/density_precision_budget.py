#!/usr/bin/env python
"""
Records what the error-budget table of the density-matrix gradient kernels measures (tests/density_precision_cases.py): per
case and quantity the kernel's error against the extended-precision stored walk, e_ref (the fp64 stored and inverse numpy walks'
own error against it), their ratio, the budget and max|q|, with the kernel that ran and the case's log10 A / A_dev.

    python scripts/density_precision_budget.py [--out profiles/r35_density_precision_budget.json]

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

from tests import density_precision_cases as DP             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r35_density_precision_budget.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    props = torch.cuda.get_device_properties(dev)
    rec = {'device': props.name, 'factor': DP.FACTOR, 'lowered': {k: list(v) for k, v in DP.LOWERED.items()}, 'cases': []}
    for case in DP.CASES:
        ref = DP.reference(case)
        entry = {'id': case.id, 'family': case.family, 'n': case.n, 'net': list(case.net), 'rows': case.rows, 'readout': case.readout,
                 'log10_amplification': ref.inputs.logA, 'past_the_inverse_guard': case.past, 'twin': case.twin, 'quantities': {}}
        try:
            got, kernel = DP.run_case(dev, case)
        except AssertionError as e:
            entry['kernel_assertion'] = str(e)[:400]
            rec['cases'].append(entry)
            print(case.id, 'KERNEL', entry['kernel_assertion'], flush=True)
            continue
        entry['kernel'] = kernel
        for q in DP.QUANTITIES:
            error, e_ref, budget = DP.measure(got, ref, q)
            entry['quantities'][q] = {'error': error, 'e_ref': e_ref, 'e_stored_walk': ref.e_c[q], 'e_inverse_walk': ref.e_np[q],
                                      'ratio': error / max(e_ref, 1e-300), 'budget': budget,
                                      'max_abs': DP._maxabs(ref.ld[q][0]), 'finite': bool(np.isfinite(got[q]).all()),
                                      'within': bool(error <= budget)}
        rec['cases'].append(entry)
        print(case.id, ' '.join(f"{q}={v['error']:.1e}/{v['ratio']:.1f}{'' if v['within'] else '!'}"
                                for q, v in entry['quantities'].items()), flush=True)
    rec['worst_ratio'] = {}
    for fam in DP.KERNEL:
        worst = max((v['ratio'], c['id'], q) for c in rec['cases'] if c['family'] == fam for q, v in c['quantities'].items())
        rec['worst_ratio'][DP.KERNEL[fam]] = {'ratio': worst[0], 'case': worst[1], 'quantity': worst[2]}
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print('worst', rec['worst_ratio'], '->', args.out)


if __name__ == '__main__':
    main()
