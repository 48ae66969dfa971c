"""
The exact noisy forward under the calibrated device noise model (qhea_model_forward_noisy_device_exact,
quanonet_amd.noise.DeviceNoise through exact_noisy_predict and evaluate_noisy(exact=True)) on the GPU: against the literal
Kraus / slot-by-slot reference of tests/device_noise_reference.py, its reductions to the uniform kernel and to the ideal model,
the non-unital fixed point of relaxation, the idle decay, the asymmetric readout, determinism and chunk independence, errors,
graph capture, the solvers.  Tolerance against the references: atol 1e-10, the one the HIP path is held to everywhere.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from tests import device_noise_reference as R
from tests import helpers as H
from tests.test_noisy_forward import _circuit, _ideal, _inputs, _model, _solver_data

pytestmark = pytest.mark.gpu
ATOL = 1e-10


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _exact(m, inputs, noise, **kw):
    from quanonet_amd.noise import exact_noisy_predict
    p, sd = exact_noisy_predict(m, inputs, noise, **kw)
    torch.cuda.synchronize()
    return p[:, 0].cpu().numpy(), sd.cpu().numpy()


def _device_noise(n, idle, seed=0):
    """per-wire parameters from a fixed seed, all different: p1 in [0.01, 0.05], p2 in [0.02, 0.1], readout01 != readout10 in
    [0.01, 0.08], t / T1 per layer in [0.01, 0.05] (T1 in [1, 2], durations 0.02 / 0.03 / 0.05), T2 in [0.5 T1, 2 T1]"""
    from quanonet_amd.noise import DeviceNoise
    rng = np.random.default_rng(1000 + 10 * n + seed)
    t1 = rng.uniform(1.0, 2.0, n)
    return DeviceNoise(p1=rng.uniform(0.01, 0.05, n), p2=rng.uniform(0.02, 0.1, n), readout01=rng.uniform(0.01, 0.08, n),
                       readout10=rng.uniform(0.01, 0.08, n), t1=t1, t2=t1 * rng.uniform(0.5, 2.0, n), t_rx=0.02, t_rot=0.03,
                       t_cx=0.05, idle=idle)


def _as_dict(dn, n):
    d = {k: [dn._at(k, q) for q in range(n)] for k in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2')}
    d.update(t_rx=dn.t_rx, t_rot=dn.t_rot, t_cx=dn.t_cx, idle=dn.idle)
    return d


def _reference(c, dn, rows):
    """(mean, std) of the first `rows` rows"""
    mean, var = R.device_moments(c['n'], c['cfgs'], c['x'][:rows], c['w'], _as_dict(dn, c['n']), c['offset'], c['coeff'],
                                 c['ham_diag'], c['ham_pauli'])
    return mean, np.sqrt(np.maximum(var, 0.0))


def _compare(m, ins, dn, k, tag):
    """the GPU's pred and shot_std of all rows against the reference on the first k"""
    c, bias = _circuit(m, ins)
    pred, sd = _exact(m, ins, dn)
    mean, std = _reference(c, dn, k)
    print(f'{tag}: max|pred err|={np.abs(pred[:k] - mean - bias).max():.2e} max|std err|={np.abs(sd[:k] - std).max():.2e} '
          f'min std={std.min():.3f}')
    np.testing.assert_allclose(pred[:k], mean + bias, rtol=0, atol=ATOL, err_msg=tag)
    np.testing.assert_allclose(sd[:k], std, rtol=0, atol=ATOL, err_msg=tag)
    assert np.all(np.isfinite(pred)) and np.all(np.isfinite(sd)) and np.all(sd >= 0.0)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_against_the_reference(dev, n, kind):
    for trainable in (True, False):
        for readout in ('Z', 'X', 'Y', 'diag'):
            m = _model(kind, n, trainable, readout, seed=n).to(dev)
            for rows in (1, 37):
                ins = _inputs(kind, rows, dev, seed=rows)
                for idle in (True, False):
                    k = min(rows, 5) if n == 6 else rows                 # n = 6: the first 5 rows of the 37 the GPU computes
                    _compare(m, ins, _device_noise(n, idle), k, f'n={n} {kind} {trainable} {readout} {rows} idle={idle}')


@pytest.mark.parametrize('readout', ['Z', 'diag'])
def test_more_than_one_workgroup_of_rows(dev, readout):
    """n = 2 holds 256 rows per workgroup: 300 rows are two workgroups, the second with a tail"""
    m = _model('quanonet', 2, True, readout, seed=2).to(dev)
    _compare(m, _inputs('quanonet', 300, dev, seed=300), _device_noise(2, True), 300, f'n=2 300 rows {readout}')


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
def test_blocks_without_sublayers(dev, n):
    """branch blocks of linear depth 0 (an encoding layer and its channels only) behind a trunk block of depth 2"""
    for readout, trainable in (('Z', True), ('Y', False)):
        m = H.quanonet(n, 3, 2, (2, 0, 1, 2), n, if_trainable_freq=trainable, scale_coeff=0.7, ham_bound=(-2.0, 3.0),
                       ham_pauli=readout).to(dev)
        ins = _inputs('quanonet', 37, dev, seed=n)
        for idle in (True, False):
            _compare(m, ins, _device_noise(n, idle, seed=1), 5 if n == 6 else 37, f'n={n} ld=0 {readout} idle={idle}')


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
def test_uniform_reduces_to_the_existing_kernel(dev, n):
    from quanonet_amd.noise import DeviceNoise, NoiseModel
    nz = NoiseModel(p1=.03, p2=.08, readout=.04)
    for kind, readout in (('quanonet', 'Z'), ('heaqnn', 'diag'), ('quanonet', 'X')):
        m = _model(kind, n, True, readout, seed=n).to(dev)
        ins = _inputs(kind, 37, dev, seed=37)
        pred, sd = _exact(m, ins, DeviceNoise.uniform(nz))
        want, want_sd = _exact(m, ins, nz)
        print(f'n={n} {kind} {readout}: max|pred diff|={np.abs(pred - want).max():.2e} max|std diff|={np.abs(sd - want_sd).max():.2e}')
        np.testing.assert_allclose(pred, want, rtol=0, atol=ATOL)
        np.testing.assert_allclose(sd, want_sd, rtol=0, atol=ATOL)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
def test_default_equals_ideal(dev, n):
    from quanonet_amd.noise import DeviceNoise
    for kind, readout in (('quanonet', 'Z'), ('heaqnn', 'Y'), ('quanonet', 'diag')):
        m = _model(kind, n, True, readout, seed=n).to(dev)
        ins = _inputs(kind, 37, dev, seed=37)
        pred, sd = _exact(m, ins, DeviceNoise())
        ideal = _ideal(m, ins).cpu().numpy()
        print(f'n={n} {kind} {readout}: max|pred - ideal|={np.abs(pred - ideal).max():.2e}')
        np.testing.assert_allclose(pred, ideal, rtol=0, atol=ATOL)
        assert np.all(np.isfinite(sd)) and np.all(sd >= 0.0)


@pytest.mark.parametrize('n', [3, 5])
def test_relaxation_is_non_unital(dev, n):
    """t_cx = 50 T1 resets every wire to |0> after its last slot: sum Z reads n on every row, whatever the inputs.  No
    depolarizing setting gives that: it pulls the read-out to the middle of the range.  shot_std is the root of a cancellation
    there and is only asked to be a number."""
    from quanonet_amd.noise import DeviceNoise
    for kind in ('quanonet', 'heaqnn'):
        m = _model(kind, n, True, 'Z', seed=n).to(dev)
        ins = _inputs(kind, 37, dev, seed=5)
        c, bias = _circuit(m, ins)
        for idle in (True, False):
            pred, sd = _exact(m, ins, DeviceNoise(t1=1.0, t2=1.0, t_cx=50.0, idle=idle))
            want = c['offset'] + n * c['coeff'] + bias
            print(f'n={n} {kind} idle={idle}: max|pred - fixed point|={np.abs(pred - want).max():.2e}')
            np.testing.assert_allclose(pred, np.full(37, want), rtol=0, atol=ATOL)
            assert np.all(np.isfinite(sd)) and np.all(sd >= 0.0)
        assert np.abs(_ideal(m, ins).cpu().numpy() - want).min() > 1e-3  # the ideal rows are somewhere else


def test_idle_matters(dev):
    from quanonet_amd.noise import DeviceNoise
    kw = dict(t1=1.0, t2=1.3, t_cx=0.05)
    m4 = _model('quanonet', 4, True, 'Z', seed=4).to(dev)
    ins = _inputs('quanonet', 37, dev, seed=4)
    on, _ = _exact(m4, ins, DeviceNoise(idle=True, **kw))
    off, _ = _exact(m4, ins, DeviceNoise(idle=False, **kw))
    print(f'n=4: max|idle on - off|={np.abs(on - off).max():.2e}')
    assert np.abs(on - off).max() > 1e-6
    m2 = _model('quanonet', 2, True, 'Z', seed=4).to(dev)                # two wires: both are in every slot
    on, sd_on = _exact(m2, ins, DeviceNoise(idle=True, **kw))
    off, sd_off = _exact(m2, ins, DeviceNoise(idle=False, **kw))
    assert np.array_equal(on, off) and np.array_equal(sd_on, sd_off)


def test_asymmetric_readout_only(dev):
    from quanonet_amd.noise import DeviceNoise
    n = 4
    m = _model('quanonet', n, True, 'diag', seed=6).to(dev)
    ins = _inputs('quanonet', 37, dev, seed=6)
    c, bias = _circuit(m, ins)
    r01, r10 = [0.02, 0.11, 0.0, 0.07], [0.09, 0.01, 0.13, 0.0]
    pred, sd = _exact(m, ins, DeviceNoise(readout01=r01, readout10=r10))
    psi = O.hea_state(c['n'], c['cfgs'], c['x'], c['w'])
    prob = psi.real ** 2 + psi.imag ** 2
    kk = np.arange(1 << n)
    conf = np.ones((1 << n, 1 << n))                                     # conf[true k, read j]
    for q in range(n):
        bk, bj = (kk[:, None] >> q) & 1, (kk[None, :] >> q) & 1
        mq = np.array([[1.0 - r01[q], r01[q]], [r10[q], 1.0 - r10[q]]])  # mq[true bit, read bit]
        conf *= mq[bk, bj]
    h = c['ham_diag']
    mean = prob @ (conf @ h)
    std = np.sqrt(prob @ (conf @ (h * h)) - mean ** 2)
    print(f'max|pred err|={np.abs(pred - mean - bias).max():.2e} max|std err|={np.abs(sd - std).max():.2e}')
    np.testing.assert_allclose(pred, mean + bias, rtol=0, atol=ATOL)
    np.testing.assert_allclose(sd, std, rtol=0, atol=ATOL)
    swapped, _ = _exact(m, ins, DeviceNoise(readout01=r10, readout10=r01))
    assert np.abs(swapped - pred).max() > 1e-3                           # the two directions are told apart


@pytest.mark.parametrize('n,kind', [(2, 'heaqnn'), (4, 'quanonet'), (6, 'heaqnn')])
def test_deterministic_and_chunk_independent(dev, n, kind):
    m = _model(kind, n, True, 'Z', seed=2).to(dev)
    ins = _inputs(kind, 1000, dev, seed=3)
    dn = _device_noise(n, True)
    a, sa = _exact(m, ins, dn)
    b, sb = _exact(m, ins, dn)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    for chunk in (7, 64, 1000):
        c, sc = _exact(m, ins, dn, chunk_rows=chunk)
        assert np.array_equal(a, c) and np.array_equal(sa, sc), chunk
    part = tuple(t[300:337] for t in ins)                                # a slice of the rows is the same rows of the whole call
    p, s = _exact(m, part, dn)
    assert np.array_equal(p, a[300:337]) and np.array_equal(s, sa[300:337])


def test_errors_launch_nothing(dev):
    from quanonet_amd import _lib
    from quanonet_amd.noise import DeviceNoise
    from tests.test_device_noise_abi import BAD, _record
    n = 5
    m = _model('quanonet', n, True, 'Z').to(dev)
    ins = _inputs('quanonet', 10, dev)
    desc, params = m.fused_desc(), H.flat(m)
    out = torch.full((10,), 123.0, dtype=torch.float64, device=dev)
    sd = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    for over in BAD:
        with pytest.raises(_lib.QheaError):
            _lib.model_forward_noisy_device_exact(desc, ins[0], ins[1], params, _record(n, **over), out=out, shot_std=sd)
    m7 = _model('heaqnn', 7, True, 'Z').to(dev)
    ins7 = _inputs('heaqnn', 10, dev)
    with pytest.raises(_lib.Unsupported):
        _lib.model_forward_noisy_device_exact(m7.fused_desc(), ins7[0], None, H.flat(m7), _record(7), out=out, shot_std=sd)
    torch.cuda.synchronize()
    assert torch.all(out == 123.0) and torch.all(sd == 456.0)
    # shot_std is optional
    nz = DeviceNoise(p1=0.01, p2=0.02, readout01=0.03, t1=1.0, t2=1.0, t_cx=0.1).params(n)
    pred, none = _lib.model_forward_noisy_device_exact(desc, ins[0], ins[1], params, nz)
    both, _ = _lib.model_forward_noisy_device_exact(desc, ins[0], ins[1], params, nz, shot_std=sd)
    torch.cuda.synchronize()
    assert none is None and torch.equal(pred, both) and torch.all(sd != 456.0)


@pytest.mark.parametrize('n', [2, 5])
def test_workspace_of_the_stated_size_is_enough(dev, n):
    """qhea_model_exact_noisy_workspace_bytes is this call's size too: a workspace of exactly that many bytes is accepted (the
    package's own workspace never has fewer than 1 MiB, which would hide a call that asks for more), one byte fewer is refused."""
    import ctypes
    from quanonet_amd import _lib
    lib = _lib.load()
    m = _model('quanonet', n, True, 'Z').to(dev)
    ins = _inputs('quanonet', 37, dev)
    desc, params, nz = m.fused_desc(), H.flat(m), _device_noise(n, True).params(n)
    want, _ = _lib.model_forward_noisy_device_exact(desc, ins[0], ins[1], params, nz)
    need = int(lib.qhea_model_exact_noisy_workspace_bytes(ctypes.byref(desc), 37))
    assert 0 < need < (1 << 20)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = torch.full((37,), 123.0, dtype=torch.float64, device=dev)

    def call(nbytes):
        with torch.cuda.device(dev):
            return lib.qhea_model_forward_noisy_device_exact(ctypes.byref(desc), 37, _lib._ptr(ins[0]), _lib._ptr(ins[1]),
                                                             _lib._ptr(params), None, ctypes.byref(nz), _lib._ptr(out), None,
                                                             _lib._ptr(ws), nbytes, _lib._stream(dev))
    assert call(need - 1) == -3
    torch.cuda.synchronize()
    assert torch.all(out == 123.0)
    assert call(need) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
def test_graph_capturable_two_launches(dev, n):
    from quanonet_amd import _lib
    m = _model('quanonet', n, True, 'Z').to(dev)
    ins = _inputs('quanonet', 100, dev)
    desc, params, nz = m.fused_desc(), H.flat(m), _device_noise(n, True).params(n)
    out = torch.empty(100, dtype=torch.float64, device=dev)
    sd = torch.empty(100, dtype=torch.float64, device=dev)
    call = lambda: _lib.model_forward_noisy_device_exact(desc, ins[0], ins[1], params, nz, out=out, shot_std=sd)
    call()                                                               # sizes the workspace outside the capture
    launches = H.kernel_launches(dev, call)
    names = [k[0] for k in launches]
    assert len(names) == 2, names
    assert 'prep_model_kernel' in names[0] and f'density_dev_fwd_kernelILi{n}EE' in names[1], names
    rows_per_wg = 256 >> (2 * n - 4)
    assert launches[1][1] == ((100 + rows_per_wg - 1) // rows_per_wg, 1, 1) and launches[1][2] == (256, 1, 1), launches


def test_solvers(dev, tmp_path):
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import DeviceNoise, exact_noisy_predict
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
    y_true = torch.tensor(data['test_output'], device=dev)
    res = s.evaluate_noisy(dn, exact=True)
    assert set(os.listdir(s.out_dir)) == files
    pred, sd = exact_noisy_predict(s.model, s.test_input, dn)
    for k, v in regression_metrics(pred, y_true).items():
        assert res[k] == v, k
    assert res['exact'] is True and res['mean_shot_std'] == float(sd.mean().item()) and res['noise'] == dn.asdict()
    res2 = s.evaluate_noisy(dn, out_name='device_metric.json', exact=True)
    assert set(os.listdir(s.out_dir)) == files | {'device_metric.json'}
    with open(os.path.join(s.out_dir, 'device_metric.json')) as f:
        assert json.load(f) == json.loads(json.dumps(res2))
    assert (open(mpath).read(), os.stat(mpath).st_mtime_ns) == before
    for call in (lambda: s.evaluate_noisy(dn), lambda: s.evaluate_noisy(dn, exact=False)):
        with pytest.raises(ValueError, match='DeviceNoise'):
            call()
    with pytest.raises(ValueError, match='DeviceNoise'):
        PTSolver(dict(cfg, train_noise=dn, prefix=str(tmp_path / 'tn')), data, device=dev, log=quiet)
    assert set(os.listdir(s.out_dir)) == files | {'device_metric.json'}
    ens = EnsembleSolver([dict(cfg, seed=k, run_id=f'm{k}', prefix=str(tmp_path / 'ens')) for k in (0, 1)], data, device=dev,
                         log=quiet)
    ens.train()
    outs = ens.evaluate_noisy(dn, exact=True)
    assert len(outs) == 2
    for mem, o in zip(ens.members, outs):
        p, _ = exact_noisy_predict(mem.model, mem.test_input, dn)
        assert o['exact'] is True and o['MSE'] == regression_metrics(p, y_true)['MSE']
        assert not os.path.exists(os.path.join(mem.out_dir, 'metric.json'))
    with pytest.raises(ValueError, match='DeviceNoise'):
        ens.evaluate_noisy(dn, exact=False)
