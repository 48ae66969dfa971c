"""
Parity record of the six density-matrix calls (qhea_model_forward_noisy_exact, ..._noisy_device_exact, the two loss_grad and the
two train_steps calls) for the library that QHEA_LIB names (default: the tree's own): SHA-256 of every output over a small grid,
and the four workspace sizes per shape.  Run it once per library and compare the outputs line by line.
  grid: QuanONet and HEAQNN; n = 2 with 65 rows (16 rows per wave of the backward kernel: a tail slot), n = 3 with 37 rows, n = 6
  (four waves per row) with 1 row, and n = 3 with a block of depth 0 and 37 rows; Z, Y and diag read-outs; train_steps over a
  ragged schedule of three steps.  The models, inputs, device setting and hash are scripts/traj_parity.py's, the setting with its
  durations scaled by 1/4 (at full length the gradient calls' guard refuses it at n = 3 and 6).
    QHEA_LIB=/path/to/libquanonet_hea.so python scripts/density_parity.py > out.txt
"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quanonet_amd import _lib                                                                         # noqa: E402
from quanonet_amd.noise import NoiseModel, _call_args                                                 # noqa: E402
from scripts.traj_parity import _device_noise, _inputs, _model, _sha                                  # noqa: E402

# (n, rows, QuanONet net, HEAQNN net); None: traj_parity's (2, 1, 1, 2) / (3, 1)
SHAPES = ((2, 65, None, None), (3, 37, None, None), (6, 1, None, None), (3, 37, (2, 0, 1, 2), (2, 0)))
SIZERS = ('exact_noisy', 'exact_noisy_grad', 'device_noisy_grad')
ADAM = dict(first_step=3, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-3)


def _bounds(rows):
    """a ragged schedule of three steps (fewer where there are fewer rows)"""
    return [0, rows // 5, rows // 2, rows] if rows >= 5 else [0, rows]


def main():
    dev = torch.device('cuda:0')
    lib = _lib.load()
    for kind in ('quanonet', 'heaqnn'):
        for n, rows, qnet, hnet in SHAPES:
            for readout in ('Z', 'Y', 'diag'):
                net = qnet if kind == 'quanonet' else hnet
                m, ins = _model(kind, n, readout, dev, net=net), _inputs(kind, dev, rows=rows)
                desc, flat, ham_diag, branch, trunk = _call_args(m, ins, 'density_parity')
                y = torch.tensor(np.random.default_rng(2).normal(size=rows), device=dev)
                P = flat.numel()
                tag = f'{kind} n={n} net={tuple(desc.net)} rows={rows} {readout}'
                ws = [int(getattr(lib, f'qhea_model_{s}_workspace_bytes')(ctypes.byref(desc), rows)) for s in SIZERS]
                # (the device forward call is sized by the uniform forward call's function)
                print(f'{tag} workspace_bytes forward={ws[0]} device_forward={ws[0]} grad={ws[1]} device_grad={ws[2]}')
                settings = (('uniform', NoiseModel(p1=0.02, p2=0.05, readout=0.03).params(), _lib.model_forward_noisy_exact,
                             _lib.model_loss_grad_noisy_exact, _lib.model_train_steps_noisy_exact),
                            ('device', _device_noise(n, scale=0.25).params(n), _lib.model_forward_noisy_device_exact,
                             _lib.model_loss_grad_noisy_device_exact, _lib.model_train_steps_noisy_device_exact))
                for name, nz, forward, loss_grad, train_steps in settings:
                    pred, sd = torch.empty(rows, device=dev, dtype=torch.float64), torch.empty(rows, device=dev, dtype=torch.float64)
                    forward(desc, branch, trunk, flat, nz, ham_diag=ham_diag, out=pred, shot_std=sd)
                    print(f'{tag} {name} forward pred={_sha(pred)} shot_std={_sha(sd)}')
                    grad, gpred = torch.zeros(P + 2, device=dev, dtype=torch.float64), torch.empty(rows, device=dev, dtype=torch.float64)
                    loss_grad(desc, branch, trunk, y, flat, nz, 1.0 / (rows + 3), grad, ham_diag=ham_diag, pred=gpred)
                    print(f'{tag} {name} loss_grad grad={_sha(grad)} pred={_sha(gpred)}')
                    bounds = _bounds(rows)
                    steps = len(bounds) - 1
                    params, m1, m2 = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
                    out = torch.zeros(steps, P + 2, device=dev, dtype=torch.float64)
                    train_steps(desc, bounds, [rows + i for i in range(steps)], branch, trunk, y, params, out, m1, m2,
                                noise=nz, ham_diag=ham_diag, **ADAM)
                    print(f'{tag} {name} train_steps steps={steps} params={_sha(params)} exp_avg={_sha(m1)} exp_avg_sq={_sha(m2)} '
                          + ' '.join(f'grad{i}={_sha(out[i])}' for i in range(steps)))
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
