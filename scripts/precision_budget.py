#!/usr/bin/env python
"""
Records what the error-budget table measures (tests/precision_cases.py): per case and quantity e_ref (the two fp64 oracles'
own error against the long-double oracle), the kernel's error, their ratio, the budget, and the kernels that ran.

    python scripts/precision_budget.py [--out profiles/r21_precision_budget.json]

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

from tests import precision_cases as PC                     # noqa: E402

CIRCUIT_Q = [('out', 'out'), ('state', 'state'), ('grad_x', 'grad_x'), ('grad_w', 'grad_w'), ('backward out', 'out')]
MODEL_Q = [('row', 'row'), ('sse', 'sse'), ('out', 'out')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_precision_budget.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    props = torch.cuda.get_device_properties(dev)
    cus = props.multi_processor_count
    rec = {'device': props.name, 'cus': cus, 'factor': PC.FACTOR, 'cases': []}
    for table, run, ref_of, quantities in ((PC.CIRCUIT_CASES, PC.run_circuit_case, lambda c: PC.circuit_reference(c, c.batch(cus)),
                                            CIRCUIT_Q),
                                           (PC.MODEL_CASES, PC.run_model_case, PC.model_reference, MODEL_Q)):
        for case in table:
            ref = ref_of(case)
            entry = {'id': case.id, 'batch': case.batch(cus) if callable(case.batch) else case.batch, 'quantities': {}}
            try:
                got, kernels = run(dev, case, cus)
            except AssertionError as e:
                entry['kernel_assertion'] = str(e)[:400]
                rec['cases'].append(entry)
                print(case.id, 'KERNELS', entry['kernel_assertion'], flush=True)
                continue
            entry['kernels'] = kernels
            for q, ld_q in quantities:
                err, e_ref, budget = PC.measure(got, ref, q, ld_q)
                entry['quantities'][q] = {'e_ref': e_ref, 'error': err, 'ratio': err / e_ref, 'budget': budget,
                                          'finite': bool(np.isfinite(got[q]).all()), 'within': bool(err <= budget)}
            rec['cases'].append(entry)
            print(case.id, ' '.join(f"{q}={v['error']:.1e}/{v['ratio']:.1f}{'' if v['within'] else '!'}"
                                    for q, v in entry['quantities'].items()), flush=True)
    worst = max((v['ratio'], c['id'], q) for c in rec['cases'] for q, v in c['quantities'].items())
    rec['worst_ratio'] = {'ratio': worst[0], 'case': worst[1], 'quantity': worst[2]}
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print('worst', rec['worst_ratio'], '->', args.out)


if __name__ == '__main__':
    main()
