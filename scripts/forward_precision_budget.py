#!/usr/bin/env python
"""
Records what the error-budget table of the exact noisy forward kernels measures (tests/forward_precision_cases.py): per case and
quantity (pred, shot_std) the kernel's error against the extended-precision channel-form reference, e_ref (the two fp64 numpy
evaluations' own error against it), their ratio, the budget and the scale the budget's floor refers to, with the kernels that ran.

    python scripts/forward_precision_budget.py [--out profiles/r38_forward_precision_budget.json]

Needs a GPU and the built libraries.  A case whose kernel names differ from the table's is recorded with its assertion's text.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402
import torch                                                # noqa: E402

from tests import forward_precision_cases as FP             # noqa: E402

UNITS = {'uniform': 'density_fwd_kernel', 'device': 'density_dev_fwd_kernel', 'wide': 'density_wide (ring, wires, readout)'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r38_forward_precision_budget.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    props = torch.cuda.get_device_properties(dev)
    rec = {'device': props.name, 'factor': FP.FACTOR, 'cap': FP.CAP, 'lowered': {k: list(v) for k, v in FP.LOWERED.items()},
           'cases': []}
    for case in FP.CASES:
        ref = FP.reference(case)
        entry = {'id': case.id, 'family': case.family, 'n': case.n, 'net': list(case.net), 'rows': case.rows,
                 'readout': case.readout, 'noise': case.noise, 'quantities': {}}
        try:
            got, kernels = FP.run_case(dev, case)
        except AssertionError as e:
            entry['kernel_assertion'] = str(e)[:400]
            rec['cases'].append(entry)
            print(case.id, 'KERNEL', entry['kernel_assertion'], flush=True)
            continue
        entry['kernels'] = kernels
        for q in FP.QUANTITIES:
            error, e_ref, budget = FP.measure(got, ref, q)
            entry['quantities'][q] = {'error': error, 'e_ref': e_ref, 'e_channel_form': ref.e_c[q], 'e_second_form': ref.e_np[q],
                                      'ratio': error / max(e_ref, 1e-300), 'budget': budget, 'error_over_budget': error / budget,
                                      'scale': FP.scale(ref, q), 'max_abs': FP._maxabs(ref.ld[q][0]),
                                      'finite': bool(np.isfinite(got[q]).all()), 'within': bool(error <= budget)}
        rec['cases'].append(entry)
        print(case.id, ' '.join(f"{q}={v['error']:.1e}/{v['ratio']:.1f}{'' if v['within'] else '!'}"
                                for q, v in entry['quantities'].items()), flush=True)
    rec['worst_ratio'], rec['tightest'] = {}, {}
    for fam, unit in UNITS.items():
        rows = [(v, c['id'], q) for c in rec['cases'] if c['family'] == fam for q, v in c['quantities'].items()]
        worst = max(rows, key=lambda r: r[0]['ratio'])
        tight = max(rows, key=lambda r: r[0]['error_over_budget'])
        rec['worst_ratio'][unit] = {'ratio': worst[0]['ratio'], 'case': worst[1], 'quantity': worst[2]}
        rec['tightest'][unit] = {'error_over_budget': tight[0]['error_over_budget'], 'case': tight[1], 'quantity': tight[2]}
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print('worst', rec['worst_ratio'], 'tightest', rec['tightest'], '->', args.out)


if __name__ == '__main__':
    main()
