"""
Parity record of the four trajectory calls (qhea_model_forward_noisy, ..._noisy_wide, ..._noisy_device, ..._noisy_device_wide)
for the library that QHEA_LIB names (default: the tree's own): SHA-256 of `pred` and `stderr` over a small grid, and the
workspace sizes per shape (lane, wide, device; for n >= 10 also device_wide).  Run it once per library and compare the outputs
line by line.
  grid: QuanONet and HEAQNN; n = 2, 6 (uniform lane call, device call), 7, 9 (uniform wide call, device call), 10, 12 (uniform wide
  call, device wide call: device_noisy_predict picks it there); 3 rows x 70 values (a full and a partial tile); expectation and
  shot mode; Z and diag read-outs; row0 = 0 and 2^32 + 5.
    QHEA_LIB=/path/to/libquanonet_hea.so python scripts/traj_parity.py > out.txt
"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quanonet_amd import _lib                                                                         # noqa: E402
from quanonet_amd.models import HEAQNNPT, QuanONetPT                                                  # noqa: E402
from quanonet_amd.noise import DeviceNoise, NoiseModel, Sampling, device_noisy_predict, noisy_predict  # noqa: E402

ROWS, VALUES = 3, 70


def _model(kind, n, readout, dev, net=None):
    """readout: 'Z', 'X', 'Y' or 'diag'; net: the net_size, by default (2, 1, 1, 2) / (3, 1)"""
    torch.manual_seed(10 * n + (kind == 'heaqnn'))
    kw = dict(scale_coeff=0.7, if_trainable_freq=True)
    if readout == 'diag':
        kw['ham_diag'] = np.random.default_rng(n).normal(size=1 << n)
    else:
        kw['ham_pauli'] = readout
    if kind == 'quanonet':
        return QuanONetPT(n, 3, 2, net or (2, 1, 1, 2), **kw).double().to(dev)
    return HEAQNNPT(n, 4, net or (3, 1), **kw).double().to(dev)


def _inputs(kind, dev, rows=ROWS):
    rng = np.random.default_rng(1)
    if kind == 'quanonet':
        return (torch.tensor(rng.uniform(-1, 1, (rows, 3)), device=dev), torch.tensor(rng.uniform(0, 1, (rows, 2)), device=dev))
    return (torch.tensor(rng.uniform(-1, 1, (rows, 4)), device=dev),)


def _device_noise(n, scale=1.0):
    """scale multiplies the durations (the gradient calls refuse the setting at scale 1: scripts/density_parity.py)"""
    rng = np.random.default_rng(100 + n)
    t1 = rng.uniform(1.0, 2.0, n)
    return DeviceNoise(p1=rng.uniform(0.02, 0.05, n), p2=rng.uniform(0.05, 0.1, n), readout01=rng.uniform(0.01, 0.05, n),
                       readout10=rng.uniform(0.04, 0.09, n), t1=t1, t2=t1 * rng.uniform(0.5, 2.0, n), t_rx=0.05 * scale,
                       t_rot=0.1 * scale, t_cx=0.3 * scale, idle=True)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def main():
    dev = torch.device('cuda:0')
    lib = _lib.load()
    for kind in ('quanonet', 'heaqnn'):
        for n in (2, 6, 7, 9, 10, 12):
            for readout in ('Z', 'diag'):
                m, ins = _model(kind, n, readout, dev), _inputs(kind, dev)
                desc = m.fused_desc()
                for shots in (0, VALUES):
                    nm = NoiseModel(p1=0.02, p2=0.05, readout=0.03, shots=shots, trajectories=VALUES, seed=(7 << 32) + 11)
                    sp = Sampling(shots=shots, trajectories=VALUES, seed=(7 << 32) + 11)
                    sizes = [int(lib.qhea_model_noisy_workspace_bytes(ctypes.byref(desc), ROWS, ctypes.byref(nm.params()))),
                             int(lib.qhea_model_noisy_wide_workspace_bytes(ctypes.byref(desc), ROWS, ctypes.byref(nm.params()))),
                             _lib.model_noisy_device_workspace_bytes(desc, ROWS, sp.params())]
                    tag = f'{kind} n={n} {readout} shots={shots}'
                    wide = f' device_wide={_lib.model_noisy_device_wide_workspace_bytes(desc, ROWS, sp.params())}' if n >= 10 else ''
                    print(f'{tag} workspace_bytes lane={sizes[0]} wide={sizes[1]} device={sizes[2]}{wide}')
                    for row0 in (0, (1 << 32) + 5):
                        pred, se = noisy_predict(m, ins, nm, row0=row0)
                        print(f'{tag} row0={row0} {"wide" if n >= 7 else "lane"} pred={_sha(pred)} stderr={_sha(se)}')
                        pred, se = device_noisy_predict(m, ins, _device_noise(n), sp, row0=row0)
                        print(f'{tag} row0={row0} device pred={_sha(pred)} stderr={_sha(se)}')
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
