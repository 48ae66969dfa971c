"""
The wide noisy forward (qhea_model_forward_noisy_wide through quanonet_amd.noise.noisy_predict, n = 7..12) on the GPU against
the numpy checker tests/noise_oracle.py.  The models are those of tests/test_noisy_forward.py; their depth is tiny, what the
sizes exercise is which index bits a gate touches:
  n = 7   the first register bit: CNOT(0 -> 6) has its control on a lane and its target in a register;
  n = 9   three register bits: CNOT(8 -> 7) has both in registers;
  n = 10  the smallest LDS kernel, one wave per workgroup;  n = 11  the ragged last pass;  n = 12  256 threads, 64 KiB of state.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import noise_oracle as NO
from tests.test_noisy_forward import _circuit, _ideal, _inputs, _model, _noisy, dev  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _readout_diag_once():
    """noise_oracle.readout_diag is a Python loop over 4^n n terms (2 s at n = 9): one evaluation per (table, q)"""
    plain = NO.readout_diag
    cached = functools.lru_cache(maxsize=None)(lambda key, n, q: plain(np.frombuffer(key), n, q))
    NO.readout_diag = lambda diag, n, q: cached(np.ascontiguousarray(diag, np.float64).tobytes(), n, q).copy()
    yield
    NO.readout_diag = plain


def _replay(c, nz, row0=0):
    return NO.replay_values(c['n'], c['cfgs'], c['x'], c['w'], nz, c['offset'], c['coeff'], c['ham_diag'], c['ham_pauli'],
                            row0=row0)


@pytest.mark.parametrize('n', [7, 8, 9, 10, 11, 12])
@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
def test_noiseless_equals_ideal(dev, n, kind):
    from quanonet_amd.noise import NoiseModel
    for trainable in (True, False):
        for readout in ('Z', 'X', 'Y', 'diag'):
            m = _model(kind, n, trainable, readout, seed=n).to(dev)
            for rows in (1, 37, 300):
                ins = _inputs(kind, rows, dev, seed=rows)
                pred, se = _noisy(m, ins, NoiseModel(seed=5))
                ideal = _ideal(m, ins).cpu().numpy()
                np.testing.assert_allclose(pred, ideal, rtol=0, atol=1e-12, err_msg=f'{trainable} {readout} {rows}')
                assert np.all(se == 0.0)


ROW0_HIGH = 2 ** 32 + 5                     # the high row word of the Philox counter
REPLAY_CASES = [(7, 'quanonet', 'diag', 0, 11), (7, 'quanonet', 'diag', 1, 11),
                (8, 'heaqnn', 'X', 0, 11), (8, 'heaqnn', 'X', 1, 11),
                (9, 'quanonet', 'diag', 0, 11), (9, 'quanonet', 'diag', 1, ROW0_HIGH),
                (10, 'heaqnn', 'Y', 0, 11), (10, 'heaqnn', 'Y', 1, 11),
                (10, 'quanonet', 'diag', 1, 11),
                (11, 'heaqnn', 'Z', 0, 11), (11, 'heaqnn', 'Z', 1, 11),
                (12, 'quanonet', 'Z', 0, 11), (12, 'quanonet', 'Z', 1, 11),
                (12, 'heaqnn', 'diag', 1, 11)]


@pytest.mark.parametrize('n,kind,readout,shots,row0', REPLAY_CASES)
def test_replay_every_row(dev, n, kind, readout, shots, row0):
    """every row's single trajectory against the gate-by-gate replay of the documented random stream.  Shot mode is compared
    for equality: the kernel's cdf order differs from numpy's sequential one only where u lies within a few ulps of a cdf edge,
    a chance below 1e-11 over the whole case set, so no row is excluded."""
    from quanonet_amd.noise import NoiseModel
    m = _model(kind, n, True, readout, seed=3).to(dev)
    ins = _inputs(kind, 37, dev, seed=4)
    c, bias = _circuit(m, ins)
    for p in (0.01, 0.2):
        nz = NoiseModel(p1=p, p2=p, readout=0.07, shots=shots, trajectories=1, seed=1234 + n)
        pred, se = _noisy(m, ins, nz, row0=row0)
        ref = _replay(c, nz, row0)[:, 0] + bias
        if shots:
            np.testing.assert_array_equal(pred, ref, err_msg=f'p={p}')
        else:
            np.testing.assert_allclose(pred, ref, rtol=0, atol=1e-12, err_msg=f'p={p}')
        assert np.all(se == 0.0)


def _ordered_mean(v):
    """the header's order: trajectories in order inside tiles of 64, then the tiles in order"""
    out = np.empty(v.shape[0])
    for b, row in enumerate(v):
        S = 0.0
        for t0 in range(0, len(row), 64):
            s = 0.0
            for x in row[t0:t0 + 64]:
                s += float(x)
            S += s
        out[b] = S / len(row)
    return out


@pytest.mark.parametrize('n,kind,T', [(8, 'quanonet', 150), (8, 'heaqnn', 64), (10, 'quanonet', 150)])
def test_replay_many_trajectories_per_row(dev, n, kind, T):
    """tiles of 64 + 64 + 22 (or one full tile): the per-row mean and standard error over the replayed values"""
    from quanonet_amd.noise import NoiseModel
    m = _model(kind, n, True, 'Z', seed=8).to(dev)
    ins = _inputs(kind, 5, dev, seed=9)
    c, bias = _circuit(m, ins)
    for shots in (0, T):
        nz = NoiseModel(p1=0.05, p2=0.1, readout=0.02, shots=shots, trajectories=T, seed=77)
        pred, se = _noisy(m, ins, nz)
        v = _replay(c, nz)
        assert v.shape == (5, T)
        np.testing.assert_allclose(pred, v.mean(axis=1) + bias, rtol=0, atol=1e-12)
        np.testing.assert_allclose(se, v.std(axis=1, ddof=1) / np.sqrt(T), rtol=0, atol=1e-12)
        if shots:                                                        # the values are exact, so the ordered sum is too
            np.testing.assert_array_equal(pred, _ordered_mean(v) + bias)


@pytest.mark.parametrize('n', [7, 10])
@pytest.mark.parametrize('shots', [0, 40])
def test_deterministic_and_chunk_independent(dev, n, shots):
    from quanonet_amd.noise import NoiseModel
    m = _model('quanonet', n, True, 'Z', seed=2).to(dev)
    ins = _inputs('quanonet', 300, dev, seed=3)
    nz = NoiseModel(p1=0.02, p2=0.05, readout=0.03, shots=shots, trajectories=3, seed=42)
    a, sa = _noisy(m, ins, nz)
    b, sb = _noisy(m, ins, nz)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    for chunk in (7, 64, 300):
        c, sc = _noisy(m, ins, nz, chunk_rows=chunk)
        assert np.array_equal(a, c) and np.array_equal(sa, sc), chunk
    d, _ = _noisy(m, ins, NoiseModel(p1=0.02, p2=0.05, readout=0.03, shots=shots, trajectories=3, seed=43))
    assert np.mean(d != a) > 0.9


@pytest.mark.parametrize('n,readout', [(7, 'Z'), (9, 'diag')])
def test_readout_noise_only(dev, n, readout):
    """p1 = p2 = 0: the ideal forward under the folded read-out"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import NoiseModel
    m = _model('quanonet', n, True, readout, seed=6).to(dev)
    ins = _inputs('quanonet', 37, dev, seed=6)
    c, bias = _circuit(m, ins)
    q = 0.1
    pred, _ = _noisy(m, ins, NoiseModel(readout=q, trajectories=1))
    if readout == 'diag':
        folded = torch.tensor(NO.readout_diag(c['ham_diag'], n, q), device=dev)
        ref = _lib.model_forward(m.fused_desc(), ins[0], ins[1], H.flat(m), ham_diag=folded).cpu().numpy()
        np.testing.assert_allclose(pred, ref, rtol=0, atol=1e-12)
    else:
        ideal = _ideal(m, ins).cpu().numpy()
        np.testing.assert_allclose(pred - bias - c['offset'], (1 - 2 * q) * (ideal - bias - c['offset']), rtol=0, atol=1e-12)


def test_errors_launch_nothing(dev):
    from quanonet_amd import _lib
    out = torch.full((10,), 123.0, dtype=torch.float64, device=dev)
    se = torch.full((10,), 456.0, dtype=torch.float64, device=dev)
    for n in (7, 12):
        m = _model('quanonet', n, True, 'Z').to(dev)
        ins = _inputs('quanonet', 10, dev)
        desc, params = m.fused_desc(), H.flat(m)
        for bad in (_lib.NoiseParams(-0.01, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.5, 0, 0, 1, 0),
                    _lib.NoiseParams(0, 0, 2.0, 0, 1, 0), _lib.NoiseParams(0, 0, 0, -3, 1, 0), _lib.NoiseParams(0, 0, 0, 0, 0, 0)):
            with pytest.raises(_lib.QheaError):
                _lib.model_forward_noisy_wide(desc, ins[0], ins[1], params, bad, out=out, stderr=se)
    m6 = _model('heaqnn', 6, True, 'Z').to(dev)
    ins6 = _inputs('heaqnn', 10, dev)
    with pytest.raises(_lib.Unsupported):
        _lib.model_forward_noisy_wide(m6.fused_desc(), ins6[0], None, H.flat(m6), _lib.NoiseParams(0.01, 0, 0, 0, 1, 0), out=out,
                                      stderr=se)
    torch.cuda.synchronize()
    assert torch.all(out == 123.0) and torch.all(se == 456.0)


@pytest.mark.parametrize('n,readout,trajectory,nodes', [(8, 'Z', 'noisy_wide_wave_kernel', 3), (12, 'Z', 'noisy_wide_lds_kernel', 3),
                                                        (8, 'diag', 'noisy_wide_wave_kernel', 4),
                                                        (12, 'diag', 'noisy_wide_lds_kernel', 4)])
def test_graph_capturable(dev, n, readout, trajectory, nodes):
    """prep, (the diag' mix,) trajectories, finish: capturable, at most four kernel nodes"""
    from quanonet_amd import _lib
    from quanonet_amd.noise import NoiseModel
    m = _model('quanonet', n, True, readout).to(dev)
    ins = _inputs('quanonet', 100, dev)
    desc, params, nz = m.fused_desc(), H.flat(m), NoiseModel(p1=0.01, readout=0.02, trajectories=3).params()
    diag = m.quantum_layer.ham_diag if readout == 'diag' else None
    out = torch.empty(100, dtype=torch.float64, device=dev)
    call = lambda: _lib.model_forward_noisy_wide(desc, ins[0], ins[1], params, nz, ham_diag=diag, out=out)
    call()                                                               # sizes the workspace outside the capture
    names = [k[0] for k in H.kernel_launches(dev, call)]
    assert len(names) == nodes <= 4, names
    for kernel in ('prep_model_kernel', trajectory, 'noisy_finish_kernel'):
        assert any(kernel in k for k in names), (kernel, names)
    assert 'prep_model_kernel' in names[0] and 'noisy_finish_kernel' in names[-1], names


def test_ptsolver_evaluate_noisy(dev, tmp_path):
    from quanonet_amd.noise import NoiseModel, noisy_predict
    from quanonet_amd.solver import PTSolver, regression_metrics
    rng = np.random.default_rng(0)

    def part(r):
        x = rng.uniform(-1, 1, (r, 4))
        return x, np.sin(x[:, 0] * x[:, 1]).reshape(-1, 1)
    trx, tro = part(300)
    tex, teo = part(250)
    data = {'train_input': trx, 'train_output': tro, 'test_input': tex, 'test_output': teo}
    cfg = {'model_type': 'HEAQNN', 'operator': 'Toy', 'num_qubits': 7, 'net_size': [2, 1], 'scale_coeff': 0.01,
           'if_trainable_freq': 'true', 'learning_rate': 1e-2, 'batch_size': 100, 'num_epochs': 2, 'seed': 0,
           'prefix': str(tmp_path / 'solo'), 'run_id': 'r0', 'eval_batch_size': 64}
    s = PTSolver(cfg, data, device=dev, log=lambda *a, **k: None)
    hist = s.train()
    s.evaluate(hist)
    assert s.model.num_qubits == 7
    mpath = os.path.join(s.out_dir, 'metric.json')
    before = (open(mpath).read(), os.stat(mpath).st_mtime_ns)
    files = set(os.listdir(s.out_dir))
    nz = NoiseModel(p1=0.01, p2=0.02, readout=0.01, shots=200, seed=9)
    res = s.evaluate_noisy(nz)
    assert set(os.listdir(s.out_dir)) == files
    pred, se = noisy_predict(s.model, s.test_input, nz)
    ref = regression_metrics(pred, torch.tensor(teo, device=dev))
    for k, v in ref.items():
        assert res[k] == v, k
    assert res['mean_stderr'] == float(se.mean().item()) > 0.0 and res['noise'] == nz.asdict()
    res2 = s.evaluate_noisy(nz, out_name='noisy_metric.json')
    assert set(os.listdir(s.out_dir)) == files | {'noisy_metric.json'}
    with open(os.path.join(s.out_dir, 'noisy_metric.json')) as f:
        assert json.load(f) == json.loads(json.dumps(res2))
    assert (open(mpath).read(), os.stat(mpath).st_mtime_ns) == before
    from quanonet_amd import _lib
    with pytest.raises(_lib.Unsupported):                                # the exact path stays n <= 6
        s.evaluate_noisy(nz, exact=True)
