"""
The exact noisy forward (qhea_model_forward_noisy_exact, quanonet_amd.noise.exact_noisy_predict, evaluate_noisy(exact=True))
on the GPU: against the density-matrix reference (tests/noise_oracle.py exact_values at n <= 5, tests/density_reference.py at
every n), noiseless = ideal, readout folding, the trajectory kernel against it, determinism and chunk independence, errors,
graph capture, the solvers.  Tolerance against the references: atol 1e-10, the one the HIP path is held to against the oracle.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from tests import density_reference as DR
from tests import helpers as H
from tests import noise_oracle as NO
from tests.test_noisy_forward import _circuit, _ideal, _inputs, _model, _noisy, _solver_data

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


def _reference(c, p1, p2, q, rows):
    """(mean, std) of the first `rows` rows; exact_values where it reaches (n <= 5), the n-general reference everywhere"""
    args = (c['n'], c['cfgs'], c['x'][:rows], c['w'], p1, p2, q, c['offset'], c['coeff'], c['ham_diag'], c['ham_pauli'])
    mean, var = DR.exact_moments(*args)
    if c['n'] <= 5:
        m2, v2 = NO.exact_values(*args)
        np.testing.assert_allclose(mean, m2, rtol=0, atol=1e-13)
        np.testing.assert_allclose(var, v2, rtol=0, atol=1e-13)
    return mean, np.sqrt(np.maximum(var, 0.0))


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_against_the_oracle(dev, n, kind):
    from quanonet_amd.noise import NoiseModel
    for trainable in (True, False):
        for readout in ('Z', 'X', 'Y', 'diag'):
            m = _model(kind, n, trainable, readout, seed=n).to(dev)
            for rows in (1, 37, 1000):
                ins = _inputs(kind, rows, dev, seed=rows)
                c, bias = _circuit(m, ins)
                for p1, p2, q in ((0.03, 0.08, 0.04), (1.0, 1.0, 1.0)):
                    if (p1, rows) == (1.0, 1000):
                        continue                                         # the corner: 1 and 37 rows
                    pred, sd = _exact(m, ins, NoiseModel(p1=p1, p2=p2, readout=q))
                    k = min(rows, 37)
                    mean, std = _reference(c, p1, p2, q, k)
                    tag = f'{trainable} {readout} {rows} p1={p1}'
                    print(f'n={n} {kind} {tag}: max|pred err|={np.abs(pred[:k] - mean - bias).max():.2e} '
                          f'max|std err|={np.abs(sd[:k] - std).max():.2e}')
                    np.testing.assert_allclose(pred[:k], mean + bias, rtol=0, atol=ATOL, err_msg=tag)
                    np.testing.assert_allclose(sd[:k], std, rtol=0, atol=ATOL, err_msg=tag)
                    assert np.all(np.isfinite(pred)) and np.all(np.isfinite(sd)) and np.all(sd >= 0.0)


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_noiseless_equals_ideal(dev, n, kind):
    """the cases of test_noisy_forward.test_noiseless_equals_ideal; shot_std against the ideal state's one-shot deviation"""
    from quanonet_amd.noise import NoiseModel
    for trainable in (True, False):
        for readout in ('Z', 'X', 'Y', 'diag'):
            m = _model(kind, n, trainable, readout, seed=n).to(dev)
            for rows in (1, 37, 1000):
                ins = _inputs(kind, rows, dev, seed=rows)
                pred, sd = _exact(m, ins, NoiseModel(seed=5))
                ideal = _ideal(m, ins).cpu().numpy()
                np.testing.assert_allclose(pred, ideal, rtol=0, atol=ATOL, err_msg=f'{trainable} {readout} {rows}')
                if rows <= 37:
                    c, bias = _circuit(m, ins)
                    psi = O.hea_state(c['n'], c['cfgs'], c['x'], c['w'])
                    NO._basis_change(psi, n, c['ham_pauli'])
                    prob = psi.real ** 2 + psi.imag ** 2
                    kk = np.arange(1 << n)
                    hv = c['ham_diag'] if c['ham_diag'] is not None else \
                        c['offset'] + c['coeff'] * (n - 2.0 * sum((kk >> i) & 1 for i in range(n)))
                    mean = prob @ hv
                    std = np.sqrt(np.maximum(prob @ (hv * hv) - mean ** 2, 0.0))
                    np.testing.assert_allclose(pred, mean + bias, rtol=0, atol=ATOL, err_msg=f'{trainable} {readout} {rows}')
                    np.testing.assert_allclose(sd, std, rtol=0, atol=ATOL, err_msg=f'{trainable} {readout} {rows}')


@pytest.mark.parametrize('readout', ['Z', 'X', 'diag'])
def test_readout_noise_only(dev, readout):
    from quanonet_amd.noise import NoiseModel
    m = _model('quanonet', 4, True, readout, seed=6).to(dev)
    ins = _inputs('quanonet', 37, dev, seed=6)
    c, bias = _circuit(m, ins)
    q = 0.13
    pred, _ = _exact(m, ins, NoiseModel(readout=q))
    ideal = _ideal(m, ins).cpu().numpy()
    if readout == 'diag':
        psi = O.hea_state(c['n'], c['cfgs'], c['x'], c['w'])
        prob = psi.real ** 2 + psi.imag ** 2
        np.testing.assert_allclose(pred, prob @ NO.readout_diag(c['ham_diag'], 4, q) + bias, rtol=0, atol=ATOL)
    else:
        np.testing.assert_allclose(pred - bias - c['offset'], (1 - 2 * q) * (ideal - bias - c['offset']), rtol=0, atol=ATOL)


@pytest.mark.parametrize('n', [2, 3, 5, 6])
@pytest.mark.parametrize('shots', [0, 20000])
def test_trajectory_kernel_against_exact(dev, n, shots):
    """
    test_noisy_forward.test_statistics_against_exact_channel with the numpy mean replaced by the GPU's exact one, plus n = 6.
    The n = 6 stream was replayed on the CPU first (noise_oracle.replay_values, two rows at a time, against
    density_reference.exact_moments): seed 1006, largest |z| over the 16 rows 2.36 in expectation mode and 2.11 in shot
    mode, shot-mode stderr sqrt(S) / shot_std within [0.990, 1.010].
    """
    from quanonet_amd.noise import NoiseModel
    m = _model('heaqnn', n, True, 'Z', seed=n + 20).to(dev)
    ins = _inputs('heaqnn', 16, dev, seed=n)
    nz = NoiseModel(p1=0.03, p2=0.08, readout=0.04, shots=shots, trajectories=20000, seed=1000 + n)
    pred, se = _noisy(m, ins, nz)
    exact, sd = _exact(m, ins, nz)
    assert np.all(se > 0)
    print(f'n={n} shots={shots}: z={(pred - exact) / se}')
    assert np.all(np.abs(pred - exact) < 5 * se), (pred - exact) / se
    if shots:
        print(f'stderr sqrt(S) / shot_std = {se * np.sqrt(shots) / sd}')
        assert np.all(np.abs(se * np.sqrt(shots) / sd - 1.0) < 0.1), se * np.sqrt(shots) / sd


@pytest.mark.parametrize('n,kind', [(5, 'quanonet'), (6, 'heaqnn'), (3, 'quanonet'), (2, 'heaqnn'), (4, 'quanonet')])
def test_deterministic_and_chunk_independent(dev, n, kind):
    from quanonet_amd.noise import NoiseModel
    m = _model(kind, n, True, 'Z', seed=2).to(dev)
    ins = _inputs(kind, 1000, dev, seed=3)
    nz = NoiseModel(p1=0.02, p2=0.05, readout=0.03)
    a, sa = _exact(m, ins, nz)
    b, sb = _exact(m, ins, nz)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    for chunk in (7, 64, 1000):
        c, sc = _exact(m, ins, nz, chunk_rows=chunk)
        assert np.array_equal(a, c) and np.array_equal(sa, sc), chunk
    part = tuple(t[300:337] for t in ins)                                # a slice of the rows is the same rows of the whole call
    p, s = _exact(m, part, nz)
    assert np.array_equal(p, a[300:337]) and np.array_equal(s, sa[300:337])
    # shots, trajectories and seed are ignored
    d, sdd = _exact(m, ins, NoiseModel(p1=0.02, p2=0.05, readout=0.03, shots=17, trajectories=3, seed=99))
    assert np.array_equal(a, d) and np.array_equal(sa, sdd)


def test_errors_launch_nothing(dev):
    from quanonet_amd import _lib
    m = _model('quanonet', 3, True, 'Z').to(dev)
    ins = _inputs('quanonet', 10, dev)
    desc, params = m.fused_desc(), H.flat(m)
    out = torch.full((10,), 123.0, dtype=torch.float64, device=dev)
    sd = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    for bad in (_lib.NoiseParams(-0.01, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.5, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
                _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0)):
        with pytest.raises(_lib.QheaError):
            _lib.model_forward_noisy_exact(desc, ins[0], ins[1], params, bad, out=out, shot_std=sd)
    m7 = _model('heaqnn', 7, True, 'Z').to(dev)
    ins7 = _inputs('heaqnn', 10, dev)
    with pytest.raises(_lib.Unsupported):
        _lib.model_forward_noisy_exact(m7.fused_desc(), ins7[0], None, H.flat(m7), _lib.NoiseParams(0.01, 0, 0, 0, 1, 0), out=out,
                                       shot_std=sd)
    torch.cuda.synchronize()
    assert torch.all(out == 123.0) and torch.all(sd == 456.0)
    # shot_std is optional
    pred, none = _lib.model_forward_noisy_exact(desc, ins[0], ins[1], params, _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0))
    both, _ = _lib.model_forward_noisy_exact(desc, ins[0], ins[1], params, _lib.NoiseParams(0.01, 0.02, 0.03, 0, 1, 0), shot_std=sd)
    torch.cuda.synchronize()
    assert none is None and torch.equal(pred, both) and torch.all(sd != 456.0)


@pytest.mark.parametrize('n', [2, 5, 6])
def test_graph_capturable_two_launches(dev, n):
    from quanonet_amd import _lib
    from quanonet_amd.noise import NoiseModel
    m = _model('quanonet', n, True, 'Z').to(dev)
    ins = _inputs('quanonet', 100, dev)
    desc, params, nz = m.fused_desc(), H.flat(m), NoiseModel(p1=0.01, p2=0.02).params()
    out = torch.empty(100, dtype=torch.float64, device=dev)
    sd = torch.empty(100, dtype=torch.float64, device=dev)
    call = lambda: _lib.model_forward_noisy_exact(desc, ins[0], ins[1], params, nz, out=out, shot_std=sd)
    call()                                                               # sizes the workspace outside the capture
    launches = H.kernel_launches(dev, call)
    names = [k[0] for k in launches]
    assert len(names) == 2, names
    assert 'prep_model_kernel' in names[0] and f'density_fwd_kernelILi{n}EE' in names[1], names
    rows_per_wg = 256 >> (2 * n - 4)
    assert launches[1][1] == ((100 + rows_per_wg - 1) // rows_per_wg, 1, 1) and launches[1][2] == (256, 1, 1), launches


def test_solver_evaluate_noisy_exact(dev, tmp_path):
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.noise import NoiseModel, exact_noisy_predict, noisy_predict
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
    y_true = torch.tensor(data['test_output'], device=dev)
    res = s.evaluate_noisy(nz, exact=True)
    assert set(os.listdir(s.out_dir)) == files
    pred, sd = exact_noisy_predict(s.model, s.test_input, nz)
    for k, v in regression_metrics(pred, y_true).items():
        assert res[k] == v, k
    assert res['exact'] is True and res['mean_shot_std'] == float(sd.mean().item()) and res['noise'] == nz.asdict()
    assert 'mean_stderr' not in res
    res2 = s.evaluate_noisy(nz, out_name='exact_metric.json', exact=True)
    assert set(os.listdir(s.out_dir)) == files | {'exact_metric.json'}
    with open(os.path.join(s.out_dir, 'exact_metric.json')) as f:
        assert json.load(f) == json.loads(json.dumps(res2))
    assert (open(mpath).read(), os.stat(mpath).st_mtime_ns) == before
    # the default is the trajectory estimate, as before
    for sampled in (s.evaluate_noisy(nz), s.evaluate_noisy(nz, exact=False)):
        p, se = noisy_predict(s.model, s.test_input, nz)
        for k, v in regression_metrics(p, y_true).items():
            assert sampled[k] == v, k
        assert sampled['mean_stderr'] == float(se.mean().item()) and 'exact' not in sampled and 'mean_shot_std' not in sampled
    assert (open(mpath).read(), os.stat(mpath).st_mtime_ns) == before
    ens = EnsembleSolver([dict(cfg, seed=k, run_id=f'm{k}', prefix=str(tmp_path / 'ens')) for k in (0, 1)], data, device=dev,
                         log=quiet)
    ens.train()
    outs = ens.evaluate_noisy(nz, exact=True)
    assert len(outs) == 2
    for mem, o in zip(ens.members, outs):
        p, _ = exact_noisy_predict(mem.model, mem.test_input, nz)
        assert o['exact'] is True and o['MSE'] == regression_metrics(p, y_true)['MSE']
        assert not os.path.exists(os.path.join(mem.out_dir, 'metric.json'))
