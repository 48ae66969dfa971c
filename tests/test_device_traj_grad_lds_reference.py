"""
CPU checks for the quantum-jump trajectory gradient at n = 10..12 (qhea_model_loss_grad_noisy_device_lds /
qhea_model_train_steps_noisy_device_lds): the host side of the new entry points (nothing is launched), the numpy reference
tests/device_traj_grad_reference.py at the new width, the Python refusals, and the arithmetic of the recorded words and of a
site's stored-bit predicate on the host (tests/native/jump_site_check.cpp).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import device_traj_grad_reference as G
from tests.conftest import ROOT
from tests.test_device_traj_grad_reference import noise
from tests.test_noisy_traj_grad_lds_reference import HIPCC

NAMES = ('qhea_model_noisy_device_lds_grad_workspace_bytes', 'qhea_noisy_device_lds_grad_max_workgroups',
         'qhea_model_loss_grad_noisy_device_lds', 'qhea_model_train_steps_noisy_device_lds')


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_symbols_and_queries(lib):
    from quanonet_amd import _lib
    from tests.test_device_noise_abi import _record
    assert lib.qhea_version() >= 610 and _lib.MIN_LIB_VERSION >= 610
    for name in NAMES:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    size, cap = lib.qhea_model_noisy_device_lds_grad_workspace_bytes, lib.qhea_noisy_device_lds_grad_max_workgroups
    sp = _lib.SamplingParams(0, 5, 1)
    desc = lambda n: _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (2, 1), 4, 0, True, 0.1, 0.0, 1.0)
    for n in range(2, 14):
        assert (cap(n) > 0) == (10 <= n <= 12), n
    assert size(ctypes.byref(desc(9)), 8, ctypes.byref(sp)) == 0
    for n in (10, 11, 12):
        d = desc(n)
        sizes = [size(ctypes.byref(d), B, ctypes.byref(sp)) for B in (0, 1, 2, 8, 64, 700, 701)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[1], (n, sizes)
        for bad in (_lib.SamplingParams(1, 5, 1), _lib.SamplingParams(0, 0, 1), _lib.SamplingParams(-1, 5, 1)):
            assert size(ctypes.byref(d), 8, ctypes.byref(bad)) == 0             # shots != 0, trajectories < 1
        assert size(ctypes.byref(d), 8, None) == 0 and size(ctypes.byref(d), -1, ctypes.byref(sp)) == 0
        # a function of the shape, the batch and T only: beyond the cap of workgroups rows cost their records alone, below it a
        # workgroup's snapshot area (2 blocks x 2^n x 16 bytes) and words as well
        T2 = _lib.SamplingParams(0, 2, 1)                                        # one item per row
        c = cap(n)
        at = lambda B: size(ctypes.byref(d), B, ctypes.byref(T2))
        assert at(3 * c) - at(2 * c) == at(4 * c) - at(3 * c) > 0
        assert at(c) - at(c // 2) >= (c // 2) * 2 * (16 << n)
    # the size takes no device setting: the query has no such argument, and the call accepts the size under any checked setting
    assert lib.qhea_model_noisy_device_lds_grad_workspace_bytes.argtypes == lib.qhea_model_noisy_device_grad_workspace_bytes.argtypes
    assert _record(10) is not None


def test_return_codes_without_a_device(lib):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    from tests.test_device_noise_abi import BAD, _record
    call, steps = lib.qhea_model_loss_grad_noisy_device_lds, lib.qhea_model_train_steps_noisy_device_lds
    sp = _lib.SamplingParams(0, 5, 1)
    desc = lambda n: _lib.make_model_desc(_lib.MODEL_HEAQNN, n, (2, 1), 4, 0, True, 0.1, 0.0, 1.0)

    def run(dd, rec, samp, batch=4, row0=0):
        return call(ctypes.byref(dd), row0, batch, None, None, None, None, None, None if rec is None else ctypes.byref(rec),
                    None if samp is None else ctypes.byref(samp), 1.0, None, None, None, 0, None)

    def run_steps(dd, rec, samp, n_steps=2, first_step=1):
        return steps(ctypes.byref(dd), n_steps, None, None, None, None, None, None, None if rec is None else ctypes.byref(rec),
                     None if samp is None else ctypes.byref(samp), None, None, 0, None, None, first_step, 1e-2, 0.9, 0.999, 1e-8, 0.0,
                     None, 0, None)

    for n in (10, 11, 12):
        d, ok = desc(n), _record(n)
        assert run(d, ok, sp, batch=0) == 0 and run_steps(d, ok, sp, n_steps=0) == 0
        assert run(d, ok, sp) == -1 and run(d, ok, sp, batch=-1) == -1 and run(d, ok, sp, row0=-1) == -1     # NULL arrays
        assert run(d, None, sp) == -1 and run(d, ok, None) == -1 and run_steps(d, ok, None) == -1           # a NULL sampling
        assert run(d, ok, _lib.SamplingParams(1, 5, 1), batch=0) == -1                                    # shot mode
        assert run(d, ok, _lib.SamplingParams(0, 0, 1), batch=0) == -1
        assert run_steps(d, ok, sp, first_step=0) == -1
        for over in BAD:
            assert run(d, _record(n, **over), sp, batch=0) == -1, over
        # the site that cannot be walked back is refused after the shared checks (an empty batch returns before it, as at 7..9)
        dead = DeviceNoise(t1=[1.0] * (n - 1) + [1e-3], t2=[1.0] * (n - 1) + [1e-3], t_rx=0.001, t_rot=0.001, t_cx=0.1, idle=False)
        assert _lib.device_noise_singular_site(n, dead.params(n)) == ('CTL', n - 1)
        buf = (ctypes.c_double * 4)()                                             # never read: refused before any launch
        with_arrays = lambda rec: call(ctypes.byref(d), 0, 4, buf, None, buf, buf, None, ctypes.byref(rec), ctypes.byref(sp), 1.0,
                                       buf, None, None, 0, None)
        assert with_arrays(ok) == -3 and with_arrays(dead.params(n)) == -1       # no workspace / the gamma = 1 site before it
    for n in (6, 9):                                                              # the range comes before the read-out and rows
        assert run(desc(n), _record(n), sp) == -2 and run_steps(desc(n), _record(n), sp) == -2
        assert run(desc(n), _record(n), _lib.SamplingParams(1, 5, 1)) == -1
    # the names of n = 7..9 keep refusing n >= 10
    old = lib.qhea_model_loss_grad_noisy_device
    assert old(ctypes.byref(desc(10)), 0, 4, None, None, None, None, None, ctypes.byref(_record(10)), ctypes.byref(sp), 1.0, None, None,
               None, 0, None) == -2


def test_reference_holds_at_the_new_width():
    """n = 10, one block of one sub-layer, one row, two trajectories: the adjoint walk is the two-term shift of the numerator"""
    n, cfgs, T = 10, [(10, 1)], 2
    rng = np.random.default_rng(110)
    x = rng.uniform(-2.0, 2.0, (1, n))
    w = rng.uniform(-np.pi, np.pi, (1, 3, n))
    nz = noise(n, rng, strong=True)
    r = G.walk(n, cfgs, x, w, nz, T, 5, 0.3, 1.2, None, 'Y', row0=2)
    cov = G.coverage(r, n, T)
    assert cov['jumps'].sum() >= T, cov
    gx, gw = G.shift_grad(n, cfgs, x, w, nz, T, 5, 0.3, 1.2, None, 'Y', row0=2)
    err = max(np.abs(gx - r['gx']).max(), np.abs(gw - r['gw']).max())
    print(f'n={n}: jumps={int(cov["jumps"].sum())} max|adjoint - shift|={err:.2e}')
    assert err <= 1e-12


def test_python_refusals_without_gpu():
    from quanonet_amd import noise as N
    from quanonet_amd.solver import DataParallelTrainer
    from tests import helpers as H
    m6, m10 = H.heaqnn(6, 3, (1, 1), 0), H.heaqnn(10, 3, (1, 1), 0)
    dn, sp = N.DeviceNoise(p1=0.01), N.Sampling(trajectories=4)
    with pytest.raises(ValueError, match='device_trajectory_loss_and_grad'):
        N.device_sampled_loss_and_grad(m10, None, None, dn, sp)
    with pytest.raises(ValueError, match='7..9'):
        N.device_sampled_loss_and_grad(m10, None, None, dn, sp)
    with pytest.raises(ValueError, match='device_noisy_loss_and_grad'):
        N.device_trajectory_loss_and_grad(m6, None, None, dn, sp)
    with pytest.raises(ValueError, match='shots'):
        N.device_trajectory_loss_and_grad(m10, None, None, dn, N.Sampling(shots=3))
    with pytest.raises(ValueError, match='DeviceNoise'):
        N.device_trajectory_loss_and_grad(m10, None, None, N.NoiseModel(), sp)
    with pytest.raises(ValueError, match='Sampling'):
        N.device_trajectory_loss_and_grad(m10, None, None, dn, N.NoiseModel())
    lin = lambda: torch.nn.Linear(2, 1).double()
    with pytest.raises(ValueError, match='train_jump_trajectories and train_trajectories are both set'):
        DataParallelTrainer(lin(), train_device_noise=dn, train_trajectories=sp, train_jump_trajectories=sp)
    with pytest.raises(ValueError, match='train_jump_trajectories and train_sampling are both set'):
        DataParallelTrainer(lin(), train_device_noise=dn, train_sampling=sp, train_jump_trajectories=sp)
    with pytest.raises(ValueError, match='train_jump_trajectories needs train_device_noise'):
        DataParallelTrainer(lin(), train_noise={'p1': 0.01}, train_jump_trajectories=sp)
    with pytest.raises(ValueError, match='shots'):
        DataParallelTrainer(lin(), train_device_noise=dn, train_jump_trajectories=N.Sampling(shots=10))
    with pytest.raises(ValueError, match='world_size'):
        DataParallelTrainer(lin(), world_size=2, train_device_noise=dn, train_jump_trajectories=sp.asdict())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_words_and_site_predicate_on_the_host(tmp_path):
    """tests/native/jump_site_check.cpp: for n = 10..12 and every site of a sub-layer, the stored-bit predicate the reverse
    walk and the re-walk apply (wire_reads_one, relax_site's as a function) against the gate-by-gate meaning of the site -- the
    wire's logical bit behind CNOT slots 0..j in pre-ring labels -- over all 2^n amplitudes and both polarities, that every pass
    holds its gate qubits, and the round trip of a segment's words"""
    exe = str(tmp_path / 'jump_site_check')
    src = os.path.join(ROOT, 'tests', 'native', 'jump_site_check.cpp')
    r = subprocess.run([HIPCC, '-O2', '-std=c++17', '-x', 'hip', '--offload-arch=gfx950', '-I', os.path.join(ROOT, 'include'),
                        '-I', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-Wno-inline-asm', src, '-o', exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=300)
    words = out.stdout.split()
    assert out.returncode == 0 and words[-2:] == ['failed', '0'], out.stdout[-2000:]
    # per n: n rotation sites and 2 n ring sites; 36 x 2 + 1 records
    assert int(words[-3]) == 3 * (10 + 11 + 12) + 73
