"""
Quantum-jump trajectories under the device noise model (qhea_model_forward_noisy_device, quanonet_amd.noise.device_noisy_predict,
evaluate_noisy(sampling=...)) on the GPU: replay of the documented random stream by tests/device_traj_reference.py (itself
checked against the density matrix in tests/test_device_traj_abi.py), statistics against the exact kernel, the ideal and the
fully-relaxed limits, determinism and chunk independence, return codes, the solvers.

Replay tolerance.  Expectation mode 1e-12: the kernels carry the state unnormalised and divide once, the replay normalises at
every damping event; both are a few hundred fp64 operations per amplitude.  Shot values are discrete and agree exactly.  A
decision u < gamma P1 or u < cdf differs between kernel and numpy only when u lies within a few ulps (1e-15 relative) of the edge:
at most 2e5 decisions per case here, so a chance below 1e-11 over the case set -- the argument of
tests/test_noisy_forward_wide.py.  No row is excluded.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import device_traj_reference as TR
from tests import helpers as H
from tests.test_device_noise_abi import BAD, _record
from tests.test_noisy_forward import _circuit, _ideal, _inputs, _model, _solver_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _strong(n, idle, seed=0):
    """all wires different; t_cx / T1 in [0.15, 0.3], so that jumps fire in most trajectories"""
    from quanonet_amd.noise import DeviceNoise
    rng = np.random.default_rng(2000 + 10 * n + seed)
    t1 = rng.uniform(1.0, 2.0, n)
    return DeviceNoise(p1=rng.uniform(0.02, 0.05, n), p2=rng.uniform(0.05, 0.1, n), readout01=rng.uniform(0.01, 0.05, n),
                       readout10=rng.uniform(0.04, 0.09, n), t1=t1, t2=t1 * rng.uniform(0.5, 2.0, n), t_rx=0.05, t_rot=0.1,
                       t_cx=0.3, idle=idle)


def _as_dict(dn, n):
    d = {k: [dn._at(k, q) for q in range(n)] for k in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2')}
    d.update(t_rx=dn.t_rx, t_rot=dn.t_rot, t_cx=dn.t_cx, idle=dn.idle)
    return d


def _traj(m, inputs, dn, sampling, **kw):
    from quanonet_amd.noise import device_noisy_predict
    p, se = device_noisy_predict(m, inputs, dn, sampling, **kw)
    torch.cuda.synchronize()
    return p[:, 0].cpu().numpy(), se.cpu().numpy()


def _exact(m, inputs, noise):
    from quanonet_amd.noise import exact_noisy_predict
    p, sd = exact_noisy_predict(m, inputs, noise)
    torch.cuda.synchronize()
    return p[:, 0].cpu().numpy(), sd.cpu().numpy()


def _replay(m, ins, dn, sampling, row0, counts=None):
    c, bias = _circuit(m, ins)
    vals = TR.replay_values(c['n'], c['cfgs'], c['x'], c['w'], _as_dict(dn, c['n']), sampling.shots, sampling.trajectories,
                            sampling.seed, c['offset'], c['coeff'], c['ham_diag'], c['ham_pauli'], row0=row0, counts=counts)
    return vals, bias


REPLAY = [(2, 'quanonet', 'Z', True, 300, 11), (2, 'heaqnn', 'Y', False, 1, 11), (3, 'heaqnn', 'X', False, 37, 11),
          (3, 'quanonet', 'diag', True, 300, 11), (6, 'quanonet', 'diag', True, 37, (1 << 32) + 5), (6, 'heaqnn', 'X', False, 300, 11),
          (7, 'heaqnn', 'Y', True, 37, 11), (7, 'quanonet', 'diag', False, 300, 11), (9, 'quanonet', 'Z', False, 37, 11),
          (9, 'heaqnn', 'diag', True, 1, 11)]


@pytest.mark.parametrize('n,kind,readout,idle,rows,row0', REPLAY)
def test_replay_every_row(dev, n, kind, readout, idle, rows, row0):
    from quanonet_amd.noise import Sampling
    m = _model(kind, n, True, readout, seed=3).to(dev)
    ins = _inputs(kind, rows, dev, seed=rows + n)
    dn = _strong(n, idle)
    # 64 trajectories of one row first: the events the case is about must fire, or it shows nothing
    counts = {}
    _replay(m, tuple(t[:1] for t in ins), dn, Sampling(trajectories=64, seed=77), row0, counts)
    assert counts['jump'] >= 1 and counts['dephasing'] >= 1 and counts['pauli'] >= 1, counts
    for shots in (0, 1):
        sp = Sampling(shots=shots, trajectories=1, seed=77)
        pred, se = _traj(m, ins, dn, sp, row0=row0)
        counts = {}
        vals, bias = _replay(m, ins, dn, sp, row0, counts)
        err = np.abs(pred - vals[:, 0] - bias)
        print(f'n={n} {kind} {readout} idle={idle} rows={rows} shots={shots}: max|err|={err.max():.2e} events={counts}')
        assert counts['jump'] >= 1 and counts['dephasing'] >= 1, counts
        assert np.all(se == 0.0)
        if shots:
            assert np.array_equal(pred, vals[:, 0] + bias)
        else:
            np.testing.assert_allclose(pred, vals[:, 0] + bias, rtol=0, atol=1e-12)


@pytest.mark.parametrize('n,kind,readout', [(2, 'heaqnn', 'Z'), (6, 'quanonet', 'Y'), (8, 'quanonet', 'diag')])
def test_replay_tiles(dev, n, kind, readout):
    """T = 150: tiles of 64 + 64 + 22; 5 rows"""
    from quanonet_amd.noise import Sampling
    m = _model(kind, n, False, readout, seed=5).to(dev)
    ins = _inputs(kind, 5, dev, seed=5)
    dn = _strong(n, True, seed=1)
    for shots in (0, 150):
        sp = Sampling(shots=shots, trajectories=150, seed=9)
        pred, se = _traj(m, ins, dn, sp, row0=2)
        vals, bias = _replay(m, ins, dn, sp, 2)
        mean, want_se = TR.mean_and_stderr(vals)
        print(f'n={n} shots={shots}: max|mean err|={np.abs(pred - mean - bias).max():.2e} max|se err|={np.abs(se - want_se).max():.2e}')
        np.testing.assert_allclose(pred, mean + bias, rtol=0, atol=1e-12)
        np.testing.assert_allclose(se, want_se, rtol=0, atol=1e-12)
        if shots:                                                        # the header's order: slots (n <= 6), then tiles
            D = 1 << n
            S = 0.0
            for t0 in range(0, 150, 64):
                tile = vals[:, t0:t0 + 64]
                if n <= 6:
                    sl = 64 // D
                    part = np.zeros(5)
                    for j in range(sl):
                        acc = np.zeros(5)
                        for t in range(j, tile.shape[1], sl):
                            acc = acc + tile[:, t]
                        part = part + acc
                else:
                    part = np.zeros(5)
                    for t in range(tile.shape[1]):
                        part = part + tile[:, t]
                S = S + part
            assert np.array_equal(pred, S / 150.0 + bias)


def _statistics(pred, se, exact, shot_std, count, shots, tag):
    z = (pred - exact) / se
    rms = float(np.sqrt(np.mean(z ** 2)))
    msg = f'{tag}: max|z|={np.abs(z).max():.2f} rms z={rms:.3f}'
    if shots:
        ratio = se * math.sqrt(count) / shot_std
        msg += f' deviation ratio in [{ratio.min():.3f}, {ratio.max():.3f}]'
    print(msg)
    assert np.all(np.abs(pred - exact) <= 5.0 * se)
    assert 0.5 <= rms <= 1.5
    if shots:
        assert np.all(np.abs(ratio - 1.0) <= 0.10)
    return z


@pytest.mark.parametrize('n,kind,readout', [(2, 'quanonet', 'Z'), (4, 'heaqnn', 'diag'), (6, 'quanonet', 'Z')])
def test_against_the_exact_kernel(dev, n, kind, readout):
    from quanonet_amd.noise import Sampling
    m = _model(kind, n, True, readout, seed=n).to(dev)
    ins = _inputs(kind, 37, dev, seed=37)
    dn = _strong(n, True, seed=2)
    exact, shot_std = _exact(m, ins, dn)
    import dataclasses
    no_relax, _ = _exact(m, ins, dataclasses.replace(dn, t1=math.inf, t2=math.inf))
    # precondition, from the two exact calls only: the relaxation is resolved at 4096 shots
    shift, se_exact = np.abs(exact - no_relax).mean(), (shot_std / math.sqrt(4096)).mean()
    print(f'n={n}: mean|relaxation shift|={shift:.4f} mean exact stderr={se_exact:.5f}')
    assert shift >= 10.0 * se_exact
    for shots in (0, 4096):
        pred, se = _traj(m, ins, dn, Sampling(shots=shots, trajectories=4096, seed=1234 + n))
        _statistics(pred, se, exact, shot_std, 4096, shots, f'n={n} {kind} {readout} shots={shots}')


def test_uniform_setting_against_the_uniform_exact_kernel(dev):
    from quanonet_amd.noise import DeviceNoise, NoiseModel, Sampling
    n = 5
    nm = NoiseModel(p1=0.03, p2=0.08, readout=0.04)
    m = _model('quanonet', n, True, 'Z', seed=n).to(dev)
    ins = _inputs('quanonet', 37, dev, seed=37)
    exact, shot_std = _exact(m, ins, nm)
    for shots in (0, 4096):
        pred, se = _traj(m, ins, DeviceNoise.uniform(nm), Sampling(shots=shots, trajectories=4096, seed=99))
        _statistics(pred, se, exact, shot_std, 4096, shots, f'uniform n={n} shots={shots}')


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6, 7, 8, 9])
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


@pytest.mark.parametrize('n', [3, 7, 9])
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


@pytest.mark.parametrize('n', [3, 7])
def test_determinism_and_chunks(dev, n):
    from quanonet_amd.noise import Sampling
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
        d, _ = _traj(m, ins, dn, Sampling(shots=shots, trajectories=70, seed=22))
        assert np.mean(a != d) > 0.9
        # row0 moves the streams with the rows
        e, _ = _traj(m, tuple(t[100:] for t in ins), dn, sp, row0=100)
        assert np.array_equal(e, a[100:])


def test_return_codes_launch_nothing(dev):
    import ctypes
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    n = 5
    m = _model('quanonet', n, True, 'Z').to(dev)
    ins = _inputs('quanonet', 10, dev)
    desc, params = m.fused_desc(), H.flat(m)
    out = torch.full((10,), 123.0, dtype=torch.float64, device=dev)
    se = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    sp = _lib.SamplingParams(0, 4, 1)
    for over in BAD:
        with pytest.raises(_lib.QheaError):
            _lib.model_forward_noisy_device(desc, ins[0], ins[1], params, _record(n, **over), sp, out=out, stderr=se)
    for bad in (_lib.SamplingParams(-3, 1, 0), _lib.SamplingParams(0, 0, 0), _lib.SamplingParams(1 << 32, 1, 0)):
        with pytest.raises(_lib.QheaError):
            _lib.model_forward_noisy_device(desc, ins[0], ins[1], params, _record(n), bad, out=out, stderr=se)
    m10 = _model('heaqnn', 10, True, 'Z').to(dev)
    ins10 = _inputs('heaqnn', 10, dev)
    with pytest.raises(_lib.Unsupported):
        _lib.model_forward_noisy_device(m10.fused_desc(), ins10[0], None, H.flat(m10), _record(10), sp, out=out, stderr=se)
    # a short workspace
    lib = _lib.load()
    need = _lib.model_noisy_device_workspace_bytes(desc, 10, sp)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rec = _record(n)
    args = (ctypes.byref(desc), 0, 10, _lib._ptr(ins[0]), _lib._ptr(ins[1]), _lib._ptr(params), None, ctypes.byref(rec),
            ctypes.byref(sp), _lib._ptr(out), _lib._ptr(se), _lib._ptr(ws))
    assert need > 0 and lib.qhea_model_forward_noisy_device(*args, need - 1, None) == -3
    assert lib.qhea_model_forward_noisy_device(*args[:-1], None, 0, None) == -3
    torch.cuda.synchronize()
    assert torch.all(out == 123.0) and torch.all(se == 456.0)
    # stderr_out is optional
    nz = DeviceNoise(p1=0.01, p2=0.02, readout01=0.03, t1=1.0, t2=1.0, t_cx=0.1).params(n)
    pred, none = _lib.model_forward_noisy_device(desc, ins[0], ins[1], params, nz, sp)
    both, _ = _lib.model_forward_noisy_device(desc, ins[0], ins[1], params, nz, sp, stderr=se)
    torch.cuda.synchronize()
    assert none is None and torch.equal(pred, both) and not torch.any(se == 456.0)


def test_graph_capturable(dev):
    from quanonet_amd import _lib
    m = _model('quanonet', 7, True, 'diag').to(dev)
    ins = _inputs('quanonet', 20, dev)
    desc, params = m.fused_desc(), H.flat(m)
    diag = m.quantum_layer.ham_diag.detach().contiguous()
    nz, sp = _strong(7, True).params(7), _lib.SamplingParams(0, 70, 4)
    want, want_se = _lib.model_forward_noisy_device(desc, ins[0], ins[1], params, nz, sp, ham_diag=diag,
                                                    stderr=torch.empty(20, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    out = torch.zeros(20, dtype=torch.float64, device=dev)
    se = torch.zeros(20, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            _lib.model_forward_noisy_device(desc, ins[0], ins[1], params, nz, sp, ham_diag=diag, out=out, stderr=se)
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(se, want_se)


def test_solvers(dev, tmp_path):
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import DeviceNoise, NoiseModel, Sampling, device_noisy_predict
    from quanonet_amd.solver import PTSolver, regression_metrics
    data = _solver_data()
    cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': 2, 'net_size': [2, 1, 2, 1], 'scale_coeff': 0.01,
           'if_trainable_freq': 'true', 'learning_rate': 1e-2, 'batch_size': 100, 'num_epochs': 2, 'seed': 0,
           'prefix': str(tmp_path / 'solo'), 'run_id': 'r0', 'eval_batch_size': 64}
    quiet = lambda *a, **k: None
    s = PTSolver(cfg, data, device=dev, log=quiet)
    hist = s.train()
    s.evaluate(hist)
    mpath = os.path.join(s.out_dir, 'metric.json')
    before = (open(mpath).read(), os.stat(mpath).st_mtime_ns)
    files = set(os.listdir(s.out_dir))
    dn = DeviceNoise(p1=[0.01, 0.02], p2=[0.03, 0.02], readout01=[0.01, 0.02], readout10=[0.03, 0.04], t1=[1.0, math.inf],
                     t2=[1.5, 4.0], t_rx=0.01, t_rot=0.01, t_cx=0.05)
    sp = Sampling(trajectories=64, seed=1)
    y_true = torch.tensor(data['test_output'], device=dev)
    res = s.evaluate_noisy(dn, sampling=sp, out_name='traj_metric.json')
    assert set(os.listdir(s.out_dir)) == files | {'traj_metric.json'}
    with open(os.path.join(s.out_dir, 'traj_metric.json')) as f:
        assert json.load(f) == json.loads(json.dumps(res))
    assert (open(mpath).read(), os.stat(mpath).st_mtime_ns) == before
    pred, se = device_noisy_predict(s.model, s.test_input, dn, sp)
    for k, v in regression_metrics(pred, y_true).items():
        assert res[k] == v, k
    assert res['mean_stderr'] == float(se.mean().item()) and res['mean_stderr'] > 0.0
    assert res['noise'] == dn.asdict() and res['sampling'] == sp.asdict() and 'exact' not in res
    with pytest.raises(ValueError, match='sampling'):
        s.evaluate_noisy(dn, exact=True, sampling=sp)
    with pytest.raises(ValueError, match='sampling'):
        s.evaluate_noisy(NoiseModel(p1=0.01), sampling=sp)
    with pytest.raises(ValueError, match='DeviceNoise'):
        s.evaluate_noisy(dn)
    ens = EnsembleSolver([dict(cfg, seed=k, run_id=f'm{k}', prefix=str(tmp_path / 'ens')) for k in (0, 1)], data, device=dev,
                         log=quiet)
    ens.train()
    outs = ens.evaluate_noisy(dn, sampling=sp)
    assert len(outs) == 2
    for mem, o in zip(ens.members, outs):
        p, _ = device_noisy_predict(mem.model, mem.test_input, dn, sp)
        assert o['sampling'] == sp.asdict() and o['MSE'] == regression_metrics(p, y_true)['MSE']
        assert not os.path.exists(os.path.join(mem.out_dir, 'metric.json'))
    with pytest.raises(ValueError, match='sampling'):
        ens.evaluate_noisy(dn, exact=True, sampling=sp)
