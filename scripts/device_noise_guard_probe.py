"""
The conditioning probe behind the guard of the device-noise gradient, with more points than
tests/test_device_noise_training_abi.py::test_conditioning_probe asserts on: the numpy helper's inverse walk against its walk
over stored forward states at log10 A_dev = 0, 4, 5, 6, 7, 8, 10, 11.99 on the circuits of DESIGN.md 7h's probe (n = 5 with 60
and 120 sub-layers, n = 6 with 20) and on n = 2, 3, 4 with 60 sub-layers, where the criterion that set the bound -- no probe at
or below it above 1e-12 -- is not met at n = 2 and n = 3.  CPU only; a few minutes.

    python scripts/device_noise_guard_probe.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.test_device_noise_training_abi import probe  # noqa: E402

if __name__ == '__main__':
    for n, blocks, ld in ((5, 30, 2), (5, 60, 2), (6, 10, 2), (2, 30, 2), (3, 30, 2), (4, 30, 2)):
        for logA, err, gmax in probe(n, blocks, ld, targets=(0.0, 4.0, 5.0, 6.0, 7.0, 8.0, 10.0, 11.99)):
            print(f'n={n} sub-layers={blocks * ld} log10A_dev={logA:.2f}: inverse walk - stored walk = {err:.2e}, '
                  f'max|g|={gmax:.2e}', flush=True)
