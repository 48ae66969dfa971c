"""
Quantum-jump trajectories under the device noise model at n = 10..12 (qhea_model_forward_noisy_device_wide, reached through
quanonet_amd.noise.device_noisy_predict and evaluate_noisy(sampling=...)) on the GPU: replay of the documented random stream by
tests/device_traj_reference.py, tiles, the ideal and the fully-relaxed limits, the uniform wide kernel as a statistical
yardstick, determinism and chunk independence, graph capture, return codes, the solver.

What the sizes exercise is which pass a site falls into: n = 10 is one wave (no barrier in a site's sum), n = 11 two waves with
the ragged last pass (bits 7..10: qubit 7 was gated in pass 1), n = 12 four waves and 64 KiB of state.  The depth is that of
tests/test_noisy_forward._model.

Replay tolerance.  Expectation mode 1e-12: the kernel carries the state unnormalised and divides once, the replay normalises at
every damping event; both are a few hundred fp64 operations per amplitude.  Shot values are discrete and agree exactly.  A
decision u < gamma P1 or u < cdf differs between kernel and numpy only when u lies within a few ulps (1e-15 relative) of the
edge.  Decisions here: every Philox call of the circuit carries at most one jump decision (n + 3 n ld calls per block; the
models of tests/test_noisy_forward._model have at most 15 n = 180 calls at n = 12), plus one cdf search in shot mode: at most
181 per trajectory, one trajectory per row, two modes of at most 37 rows, six cases: below 1e5 decisions in all, so a chance
below 1e-10 over the case set -- the argument of tests/test_device_traj.py.  No row is excluded.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import device_traj_reference as TR
from tests import helpers as H
from tests.test_device_noise_abi import _record
from tests.test_device_traj import _replay, _statistics, _strong, _traj
from tests.test_noisy_forward import _ideal, _inputs, _model, _solver_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


REPLAY = [(10, 'heaqnn', 'Y', True, 37, 11), (10, 'quanonet', 'diag', False, 37, (1 << 32) + 5), (11, 'heaqnn', 'Z', True, 37, 11),
          (11, 'quanonet', 'X', False, 5, 11), (12, 'quanonet', 'Z', True, 37, 11), (12, 'heaqnn', 'diag', False, 5, 11)]


@pytest.mark.parametrize('n,kind,readout,idle,rows,row0', REPLAY)
def test_replay_every_row(dev, n, kind, readout, idle, rows, row0):
    from quanonet_amd.noise import Sampling
    m = _model(kind, n, True, readout, seed=3).to(dev)
    ins = _inputs(kind, rows, dev, seed=rows + n)
    dn = _strong(n, idle)
    # 8 trajectories of one row first, from the replay alone: the events the case is about must fire, or it shows nothing
    counts = {}
    _replay(m, tuple(t[:1] for t in ins), dn, Sampling(trajectories=8, seed=77), row0, counts)
    assert counts['jump'] >= 1 and counts['dephasing'] >= 1 and counts['pauli'] >= 1, counts
    for shots in (0, 1):
        sp = Sampling(shots=shots, trajectories=1, seed=77)
        pred, se = _traj(m, ins, dn, sp, row0=row0)
        counts = {}
        vals, bias = _replay(m, ins, dn, sp, row0, counts)
        err = np.abs(pred - vals[:, 0] - bias)
        print(f'n={n} {kind} {readout} idle={idle} rows={rows} shots={shots}: max|err|={err.max():.2e} events={counts}')
        assert counts['jump'] >= 1 and counts['dephasing'] >= 1 and counts['pauli'] >= 1, counts
        assert np.all(se == 0.0)
        if shots:
            assert np.array_equal(pred, vals[:, 0] + bias)
        else:
            np.testing.assert_allclose(pred, vals[:, 0] + bias, rtol=0, atol=1e-12)


@pytest.mark.parametrize('shots', [0, 150])
def test_replay_tiles(dev, shots):
    """T = 150: tiles of 64 + 64 + 22; 5 rows.  (One case per mode: the replay of 750 trajectories is the case's time.)"""
    from quanonet_amd.noise import Sampling
    n = 10
    m = _model('quanonet', n, False, 'Z', seed=5).to(dev)
    ins = _inputs('quanonet', 5, dev, seed=5)
    dn = _strong(n, True, seed=1)
    sp = Sampling(shots=shots, trajectories=150, seed=9)
    pred, se = _traj(m, ins, dn, sp, row0=2)
    vals, bias = _replay(m, ins, dn, sp, 2)
    mean, want_se = TR.mean_and_stderr(vals)
    print(f'n={n} shots={shots}: max|mean err|={np.abs(pred - mean - bias).max():.2e} max|se err|={np.abs(se - want_se).max():.2e}')
    np.testing.assert_allclose(pred, mean + bias, rtol=0, atol=1e-12)
    np.testing.assert_allclose(se, want_se, rtol=0, atol=1e-12)
    if shots:                                                            # the header's order: trajectories, then tiles
        S = 0.0
        for t0 in range(0, 150, 64):
            tile = vals[:, t0:t0 + 64]
            part = np.zeros(5)
            for t in range(tile.shape[1]):
                part = part + tile[:, t]
            S = S + part
        assert np.array_equal(pred, S / 150.0 + bias)


@pytest.mark.parametrize('n', [10, 11, 12])
def test_default_equals_ideal(dev, n):
    from quanonet_amd.noise import DeviceNoise, Sampling
    for kind, readout in (('quanonet', 'Z'), ('heaqnn', 'diag'), ('quanonet', 'Y')):
        m = _model(kind, n, True, readout, seed=n).to(dev)
        for rows in (1, 37, 300):
            ins = _inputs(kind, rows, dev, seed=rows)
            pred, se = _traj(m, ins, DeviceNoise(), Sampling(seed=5))
            ideal = _ideal(m, ins).cpu().numpy()
            np.testing.assert_allclose(pred, ideal, rtol=0, atol=1e-12, err_msg=f'{kind} {readout} {rows}')
            assert np.all(se == 0.0)


@pytest.mark.parametrize('n', [10, 12])
def test_full_relaxation_ends_in_the_ground_state(dev, n):
    """t_cx = 50 t1: every wire's last slot resets it, so every trajectory of every row reads |0..0>"""
    from quanonet_amd.noise import DeviceNoise, Sampling
    for kind in ('quanonet', 'heaqnn'):
        m = _model(kind, n, True, 'Z', seed=n).to(dev)
        q = m.quantum_layer
        bias = float(m.bias.item()) if kind == 'quanonet' else 0.0
        want = q.ham_offset + n * q.ham_coeff + bias
        dn = DeviceNoise(p1=0.02, p2=0.05, t1=1.0, t2=1.5, t_rx=0.1, t_rot=0.1, t_cx=50.0)
        for shots in (0, 20):
            pred, se = _traj(m, _inputs(kind, 37, dev), dn, Sampling(shots=shots, trajectories=20, seed=3))
            np.testing.assert_allclose(pred, want, rtol=0, atol=1e-10)
            assert np.all(se <= 1e-7)                                    # the variance's own rounding


def test_pauli_only_device_against_the_uniform_wide_kernel(dev):
    """two streams, one expectation: every row within 5 joint standard errors, rms z in [0.5, 1.5] (the bounds of _statistics)"""
    from quanonet_amd.noise import DeviceNoise, NoiseModel, Sampling, noisy_predict
    n = 10
    m = _model('quanonet', n, True, 'Z', seed=n).to(dev)
    ins = _inputs('quanonet', 37, dev, seed=37)
    a, sa = _traj(m, ins, DeviceNoise.uniform(NoiseModel(p1=0.03, p2=0.08, readout=0.04)), Sampling(trajectories=1024, seed=99))
    b, sb = noisy_predict(m, ins, NoiseModel(p1=0.03, p2=0.08, readout=0.04, trajectories=1024, seed=1234))
    torch.cuda.synchronize()
    b, sb = b[:, 0].cpu().numpy(), sb.cpu().numpy()
    joint = np.sqrt(sa ** 2 + sb ** 2)
    z = _statistics(a, joint, b, None, 1024, 0, f'pauli-only n={n}')
    assert z.shape == (37,)


def test_determinism_and_chunks(dev):
    from quanonet_amd.noise import Sampling
    n = 11
    m = _model('quanonet', n, True, 'Z', seed=n).to(dev)
    ins = _inputs('quanonet', 300, dev, seed=300)
    dn = _strong(n, True)
    for shots in (0, 70):
        sp = Sampling(shots=shots, trajectories=70, seed=21)
        a, sa = _traj(m, ins, dn, sp)
        b, sb = _traj(m, ins, dn, sp)
        assert np.array_equal(a, b) and np.array_equal(sa, sb)
        for chunk in (7, 64, 300):
            c, sc = _traj(m, ins, dn, sp, chunk_rows=chunk)
            assert np.array_equal(a, c) and np.array_equal(sa, sc), chunk


def test_graph_capturable(dev):
    from quanonet_amd import _lib
    n = 10
    m = _model('quanonet', n, True, 'diag').to(dev)
    ins = _inputs('quanonet', 20, dev)
    desc, params = m.fused_desc(), H.flat(m)
    diag = m.quantum_layer.ham_diag.detach().contiguous()
    nz, sp = _strong(n, True).params(n), _lib.SamplingParams(0, 70, 4)
    want, want_se = _lib.model_forward_noisy_device_wide(desc, ins[0], ins[1], params, nz, sp, ham_diag=diag,
                                                         stderr=torch.empty(20, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    out = torch.zeros(20, dtype=torch.float64, device=dev)
    se = torch.zeros(20, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            _lib.model_forward_noisy_device_wide(desc, ins[0], ins[1], params, nz, sp, ham_diag=diag, out=out, stderr=se)
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(se, want_se)


def test_return_codes_on_the_device(dev):
    from quanonet_amd import _lib
    n = 10
    m = _model('quanonet', n, True, 'Z').to(dev)
    ins = _inputs('quanonet', 10, dev)
    desc, params = m.fused_desc(), H.flat(m)
    out = torch.full((10,), 123.0, dtype=torch.float64, device=dev)
    se = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    sp = _lib.SamplingParams(0, 4, 1)
    m9 = _model('heaqnn', 9, True, 'Z').to(dev)
    ins9 = _inputs('heaqnn', 10, dev)
    with pytest.raises(_lib.Unsupported):
        _lib.model_forward_noisy_device_wide(m9.fused_desc(), ins9[0], None, H.flat(m9), _record(9), sp, out=out, stderr=se)
    # a short workspace
    lib = _lib.load()
    need = _lib.model_noisy_device_wide_workspace_bytes(desc, 10, sp)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rec = _record(n)
    args = (ctypes.byref(desc), 0, 10, _lib._ptr(ins[0]), _lib._ptr(ins[1]), _lib._ptr(params), None, ctypes.byref(rec),
            ctypes.byref(sp), _lib._ptr(out), _lib._ptr(se), _lib._ptr(ws))
    assert need > 0 and lib.qhea_model_forward_noisy_device_wide(*args, need - 1, None) == -3
    assert lib.qhea_model_forward_noisy_device_wide(*args[:-1], None, 0, None) == -3
    torch.cuda.synchronize()
    assert torch.all(out == 123.0) and torch.all(se == 456.0)
    assert lib.qhea_model_forward_noisy_device_wide(*args, need, None) == 0
    torch.cuda.synchronize()
    assert not torch.any(out == 123.0) and not torch.any(se == 456.0)


def test_solver(dev, tmp_path):
    from quanonet_amd.noise import Sampling, device_noisy_predict
    from quanonet_amd.solver import PTSolver, regression_metrics
    n = 10
    data = _solver_data(rows_train=100, rows_test=40)
    cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': n, 'net_size': [2, 1, 2, 1], 'scale_coeff': 0.01,
           'if_trainable_freq': 'true', 'learning_rate': 1e-2, 'batch_size': 100, 'num_epochs': 1, 'seed': 0,
           'prefix': str(tmp_path / 'solo'), 'run_id': 'r0', 'eval_batch_size': 64}
    s = PTSolver(cfg, data, device=dev, log=lambda *a, **k: None)
    s.evaluate(s.train())
    dn, sp = _strong(n, True), Sampling(trajectories=64, seed=1)
    res = s.evaluate_noisy(dn, sampling=sp, out_name='traj_metric.json')
    with open(os.path.join(s.out_dir, 'traj_metric.json')) as f:
        assert json.load(f) == json.loads(json.dumps(res))
    pred, se = device_noisy_predict(s.model, s.test_input, dn, sp)
    y_true = torch.tensor(data['test_output'], device=dev)
    for k, v in regression_metrics(pred, y_true).items():
        assert res[k] == v, k
    assert res['mean_stderr'] == float(se.mean().item()) and res['mean_stderr'] > 0.0
    assert res['noise'] == dn.asdict() and res['sampling'] == sp.asdict()
