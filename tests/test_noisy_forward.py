"""
The noisy forward (qhea_model_forward_noisy, quanonet_amd.noise, PTSolver.evaluate_noisy) on the GPU against the numpy
checker tests/noise_oracle.py: noiseless = ideal, trajectory replay of the documented random stream, determinism and chunk
independence, statistics against the exact density-matrix channel, readout folding, the ibm_inference.py workload, errors.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from tests import helpers as H
from tests import noise_oracle as NO

pytestmark = pytest.mark.gpu
PAULIS = ('Z', 'X', 'Y')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _model(kind, n, trainable, readout, seed=0):
    """fp64 model on the CPU; readout in 'Z', 'X', 'Y', 'diag'"""
    kw = dict(if_trainable_freq=trainable, scale_coeff=0.7, ham_bound=(-2.0, 3.0))
    if readout == 'diag':
        kw['ham_diag'] = np.random.default_rng(seed + 50).normal(size=1 << n)
    else:
        kw['ham_pauli'] = readout
    if kind == 'quanonet':
        m = H.quanonet(n, 3, 2, (2, 1, 1, 2), seed, **kw)
    else:
        m = H.heaqnn(n, 4, (3, 1), seed, **kw)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(seed + 7)
        for name, p in m.named_parameters():
            if name.endswith('freq.weights'):
                p.copy_(0.5 + torch.rand(p.shape, generator=gen, dtype=torch.float64))
    return m


def _inputs(kind, rows, dev, seed=1):
    rng = np.random.default_rng(seed)
    if kind == 'quanonet':
        return (torch.tensor(rng.uniform(-1, 1, (rows, 3)), device=dev), torch.tensor(rng.uniform(0, 1, (rows, 2)), device=dev))
    return (torch.tensor(rng.uniform(-1, 1, (rows, 4)), device=dev),)


def _circuit(m, inputs):
    """(oracle circuit kwargs, bias) of a model on its inputs"""
    from quanonet_amd.models import QuanONetPT
    n = m.num_qubits
    with torch.no_grad():
        if isinstance(m, QuanONetPT):
            x = torch.cat([m.trunk_freq(inputs[1]), m.branch_freq(inputs[0])], dim=1)
            cfgs = O.block_configs_quanonet(n, m.net_size)
            bias = float(m.bias.item())
        else:
            x = m.freq(inputs[0])
            cfgs = O.block_configs_heaqnn(n, m.net_size)
            bias = 0.0
    q = m.quantum_layer
    diag = q.ham_diag.cpu().numpy() if q.use_full_ham else None
    return dict(n=n, cfgs=cfgs, x=x.cpu().numpy(), w=q.ansatz_weights.detach().cpu().numpy(), offset=q.ham_offset,
                coeff=q.ham_coeff, ham_diag=diag, ham_pauli=PAULIS[q.ham_pauli]), bias


def _ideal(m, inputs):
    from quanonet_amd import _lib
    q = m.quantum_layer
    diag = q.ham_diag if q.use_full_ham else None
    return _lib.model_forward(m.fused_desc(), inputs[0], inputs[1] if len(inputs) > 1 else None, H.flat(m), ham_diag=diag)


def _noisy(m, inputs, noise, **kw):
    from quanonet_amd.noise import noisy_predict
    p, se = noisy_predict(m, inputs, noise, **kw)
    torch.cuda.synchronize()
    return p[:, 0].cpu().numpy(), se.cpu().numpy()


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_noiseless_equals_ideal(dev, n, kind):
    from quanonet_amd.noise import NoiseModel
    for trainable in (True, False):
        for readout in ('Z', 'X', 'Y', 'diag'):
            m = _model(kind, n, trainable, readout, seed=n).to(dev)
            for rows in (1, 37, 1000):
                ins = _inputs(kind, rows, dev, seed=rows)
                pred, se = _noisy(m, ins, NoiseModel(seed=5))
                ideal = _ideal(m, ins).cpu().numpy()
                np.testing.assert_allclose(pred, ideal, rtol=0, atol=1e-12, err_msg=f'{trainable} {readout} {rows}')
                assert np.all(se == 0.0)
                if rows <= 37:
                    c, bias = _circuit(m, ins)
                    ref = O.hea_forward(c['n'], c['cfgs'], c['x'], c['w'], c['offset'], c['coeff'], c['ham_diag'],
                                        ham_pauli=c['ham_pauli']) + bias
                    np.testing.assert_allclose(pred, ref, rtol=0, atol=1e-12, err_msg=f'{trainable} {readout} {rows}')


@pytest.mark.parametrize('n,kind,readout', [(2, 'quanonet', 'Z'), (3, 'heaqnn', 'X'), (4, 'quanonet', 'diag'),
                                            (5, 'quanonet', 'Y'), (6, 'heaqnn', 'Z'), (5, 'heaqnn', 'diag')])
def test_replay_every_row(dev, n, kind, readout):
    from quanonet_amd.noise import NoiseModel
    m = _model(kind, n, True, readout, seed=3).to(dev)
    ins = _inputs(kind, 37, dev, seed=4)
    c, bias = _circuit(m, ins)
    for p in (0.01, 0.2):
        for shots in (0, 1):
            nz = NoiseModel(p1=p, p2=p, readout=0.07, shots=shots, trajectories=1, seed=1234 + n)
            pred, se = _noisy(m, ins, nz, row0=11)
            ref = NO.replay_values(c['n'], c['cfgs'], c['x'], c['w'], nz, c['offset'], c['coeff'], c['ham_diag'],
                                   c['ham_pauli'], row0=11)[:, 0] + bias
            if shots:
                np.testing.assert_array_equal(pred, ref, err_msg=f'p={p}')
            else:
                np.testing.assert_allclose(pred, ref, rtol=0, atol=1e-12, err_msg=f'p={p}')
            assert np.all(se == 0.0)


def test_replay_many_trajectories_per_row(dev):
    """T > one tile and several slots per wave: the oracle's per-row mean over the replayed trajectories"""
    from quanonet_amd.noise import NoiseModel
    m = _model('quanonet', 3, True, 'Z', seed=8).to(dev)
    ins = _inputs('quanonet', 5, dev, seed=9)
    c, bias = _circuit(m, ins)
    for shots in (0, 150):
        nz = NoiseModel(p1=0.05, p2=0.1, readout=0.02, shots=shots, trajectories=150, seed=77)
        pred, se = _noisy(m, ins, nz)
        v = NO.replay_values(c['n'], c['cfgs'], c['x'], c['w'], nz, c['offset'], c['coeff'], c['ham_diag'], c['ham_pauli'])
        np.testing.assert_allclose(pred, v.mean(axis=1) + bias, rtol=0, atol=1e-12)
        np.testing.assert_allclose(se, v.std(axis=1, ddof=1) / np.sqrt(v.shape[1]), rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize('shots', [0, 40])
def test_deterministic_and_chunk_independent(dev, shots):
    from quanonet_amd.noise import NoiseModel
    m = _model('quanonet', 5, True, 'Z', seed=2).to(dev)
    ins = _inputs('quanonet', 1000, dev, seed=3)
    nz = NoiseModel(p1=0.02, p2=0.05, readout=0.03, shots=shots, trajectories=70, seed=42)
    a, sa = _noisy(m, ins, nz)
    b, sb = _noisy(m, ins, nz)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    for chunk in (7, 64, 1000):
        c, sc = _noisy(m, ins, nz, chunk_rows=chunk)
        assert np.array_equal(a, c) and np.array_equal(sa, sc), chunk
    # a slice of the rows with its global row0 is the same rows of the whole call
    from quanonet_amd.noise import noisy_predict
    part = tuple(t[300:337] for t in ins)
    p, s = noisy_predict(m, part, nz, row0=300)
    assert np.array_equal(p[:, 0].cpu().numpy(), a[300:337]) and np.array_equal(s.cpu().numpy(), sa[300:337])
    d, _ = _noisy(m, ins, NoiseModel(p1=0.02, p2=0.05, readout=0.03, shots=shots, trajectories=70, seed=43))
    assert np.mean(d != a) > 0.9


@pytest.mark.parametrize('n', [2, 3, 5])
@pytest.mark.parametrize('shots', [0, 20000])
def test_statistics_against_exact_channel(dev, n, shots):
    from quanonet_amd.noise import NoiseModel
    m = _model('heaqnn', n, True, 'Z', seed=n + 20).to(dev)
    ins = _inputs('heaqnn', 16, dev, seed=n)
    c, bias = _circuit(m, ins)
    nz = NoiseModel(p1=0.03, p2=0.08, readout=0.04, shots=shots, trajectories=20000, seed=1000 + n)
    pred, se = _noisy(m, ins, nz)
    mean, var = NO.exact_values(c['n'], c['cfgs'], c['x'], c['w'], nz.p1, nz.p2, nz.readout, c['offset'], c['coeff'])
    assert np.all(se > 0)
    assert np.all(np.abs(pred - bias - mean) < 5 * se), (pred - bias - mean) / se
    if shots:
        exact_se = np.sqrt(var / shots)
        assert np.all(np.abs(se / exact_se - 1.0) < 0.1), se / exact_se


@pytest.mark.parametrize('readout', ['Z', 'X', 'diag'])
def test_readout_noise_only(dev, readout):
    from quanonet_amd.noise import NoiseModel
    m = _model('quanonet', 4, True, readout, seed=6).to(dev)
    ins = _inputs('quanonet', 37, dev, seed=6)
    c, bias = _circuit(m, ins)
    q = 0.13
    pred, _ = _noisy(m, ins, NoiseModel(readout=q, trajectories=1))
    ideal = _ideal(m, ins).cpu().numpy()
    if readout == 'diag':
        mean, _ = NO.exact_values(c['n'], c['cfgs'], c['x'], c['w'], 0.0, 0.0, q, ham_diag=c['ham_diag'])
        np.testing.assert_allclose(pred, mean + bias, rtol=0, atol=1e-12)
    else:
        np.testing.assert_allclose(pred - bias - c['offset'], (1 - 2 * q) * (ideal - bias - c['offset']), rtol=0, atol=1e-12)


def _hardware_model(dev):
    """ibm_inference.py's model and inputs: the shipped Antideriv Q2 Net5-1-5-1, 100 rows (branch cos(pi linspace(0,1,10)),
    trunk linspace(0,1,100))"""
    from quanonet_amd.models import QuanONetPT
    from quanonet_amd.checkpoint import ms_to_pt_state
    st = dict(np.load(os.path.join(H.GOLDEN, 'antideriv_q2.npz')))
    m = QuanONetPT(2, 10, 1, (5, 1, 5, 1), scale_coeff=0.001, if_trainable_freq=True, ham_bound=(-5.0, 5.0))
    m.load_state_dict({k: torch.tensor(v, dtype=torch.float64) for k, v in ms_to_pt_state(st, 2, (5, 1, 5, 1)).items()})
    branch = np.tile(np.cos(np.pi * np.linspace(0, 1, 10)), (100, 1))
    trunk = np.linspace(0, 1, 100).reshape(-1, 1)
    return m.to(dev), (torch.tensor(branch, device=dev), torch.tensor(trunk, device=dev))


def test_hardware_workload(dev):
    from quanonet_amd.noise import NoiseModel
    m, ins = _hardware_model(dev)
    ideal = _ideal(m, ins).cpu().numpy()
    pred, _ = _noisy(m, ins, NoiseModel())
    np.testing.assert_allclose(pred, ideal, rtol=0, atol=1e-12)
    pred, se = _noisy(m, ins, NoiseModel(shots=10000, seed=2024))
    assert np.all(se > 0)
    assert np.all(np.abs(pred - ideal) < 5 * se), (pred - ideal) / se


def test_errors_launch_nothing(dev):
    from quanonet_amd import _lib
    m = _model('quanonet', 3, True, 'Z').to(dev)
    ins = _inputs('quanonet', 10, dev)
    desc, params = m.fused_desc(), H.flat(m)
    out = torch.full((10,), 123.0, dtype=torch.float64, device=dev)
    se = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    for bad in (_lib.NoiseParams(-0.01, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.5, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
                _lib.NoiseParams(0, 0, 0, -3, 1, 0), _lib.NoiseParams(0, 0, 0, 0, 0, 0)):
        with pytest.raises(_lib.QheaError):
            _lib.model_forward_noisy(desc, ins[0], ins[1], params, bad, out=out, stderr=se)
    m7 = _model('heaqnn', 7, True, 'Z').to(dev)
    ins7 = _inputs('heaqnn', 10, dev)
    with pytest.raises(_lib.Unsupported):
        _lib.model_forward_noisy(m7.fused_desc(), ins7[0], None, H.flat(m7), _lib.NoiseParams(0.01, 0, 0, 0, 1, 0), out=out,
                                 stderr=se)
    torch.cuda.synchronize()
    assert torch.all(out == 123.0) and torch.all(se == 456.0)


def test_graph_capturable_three_launches(dev):
    from quanonet_amd import _lib
    from quanonet_amd.noise import NoiseModel
    m = _model('quanonet', 5, True, 'Z').to(dev)
    ins = _inputs('quanonet', 100, dev)
    desc, params, nz = m.fused_desc(), H.flat(m), NoiseModel(p1=0.01, trajectories=3).params()
    out = torch.empty(100, dtype=torch.float64, device=dev)
    _lib.model_forward_noisy(desc, ins[0], ins[1], params, nz, out=out)          # sizes the workspace outside the capture
    names = [k[0] for k in H.kernel_launches(dev, lambda: _lib.model_forward_noisy(desc, ins[0], ins[1], params, nz, out=out))]
    assert len(names) == 3, names
    for kernel in ('prep_model_kernel', 'noisy_fwd_kernel', 'noisy_finish_kernel'):
        assert any(kernel in k for k in names), (kernel, names)


def _solver_data(rows_train=300, rows_test=250):
    rng = np.random.default_rng(0)
    def part(r):
        b = rng.uniform(-1, 1, (r, 10))
        t = rng.uniform(0, 1, (r, 1))
        return b, t, (np.sin(t[:, 0] * b[:, 0])).reshape(-1, 1)
    trb, trt, tro = part(rows_train)
    teb, tet, teo = part(rows_test)
    return {'train_branch_input': trb, 'train_trunk_input': trt, 'train_output': tro,
            'test_branch_input': teb, 'test_trunk_input': tet, 'test_output': teo}


def test_ptsolver_evaluate_noisy(dev, tmp_path):
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import NoiseModel, noisy_predict
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
    nz = NoiseModel(p1=0.01, p2=0.02, readout=0.01, shots=200, seed=9)
    res = s.evaluate_noisy(nz)
    assert set(os.listdir(s.out_dir)) == files
    pred, se = noisy_predict(s.model, s.test_input, nz)
    ref = regression_metrics(pred, torch.tensor(data['test_output'], device=dev))
    for k, v in ref.items():
        assert res[k] == v, k
    assert res['mean_stderr'] == float(se.mean().item()) and res['noise'] == nz.asdict()
    res2 = s.evaluate_noisy(nz, out_name='noisy_metric.json')
    assert set(os.listdir(s.out_dir)) == files | {'noisy_metric.json'}
    with open(os.path.join(s.out_dir, 'noisy_metric.json')) as f:
        assert json.load(f) == json.loads(json.dumps(res2))
    assert (open(mpath).read(), os.stat(mpath).st_mtime_ns) == before
    ens = EnsembleSolver([dict(cfg, seed=k, run_id=f'm{k}', prefix=str(tmp_path / 'ens')) for k in (0, 1)], data, device=dev,
                         log=quiet)
    ens.train()
    outs = ens.evaluate_noisy(nz)
    assert len(outs) == 2
    for mem, o in zip(ens.members, outs):
        p, _ = noisy_predict(mem.model, mem.test_input, nz)
        assert o['MSE'] == regression_metrics(p, torch.tensor(data['test_output'], device=dev))['MSE']
        assert not os.path.exists(os.path.join(mem.out_dir, 'metric.json'))
