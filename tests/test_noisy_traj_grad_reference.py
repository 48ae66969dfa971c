"""
CPU checks of the sampled-trajectory gradient (qhea_model_loss_grad_noisy_wide / qhea_model_train_steps_noisy_wide): the numpy
reference tests/noisy_traj_grad_reference.py against the ideal oracle, its adjoint form against central differences of the
replay, the unbiasedness condition the GPU test holds the kernel to (same seeds, same T) on the reference alone, and the C
ABI's symbols and argument checks (nothing is launched, no GPU needed).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import noisy_traj_grad_reference as TG
from tests.conftest import ROOT

NEW = ('qhea_model_noisy_wide_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_wide', 'qhea_model_train_steps_noisy_wide')
READOUTS = ('Z', 'X', 'Y', 'diag')
# The unbiasedness check: K seeds of T trajectories each, at rates where a trajectory's derivative scatters visibly
UNBIASED = dict(n=7, net=(1, 1), K=16, T=64, seeds=tuple(range(100, 116)), rates=(0.05, 0.1, 0.05), sigmas=5.0)


def noise_model(p, T=1, seed=0):
    from quanonet_amd.noise import NoiseModel
    return NoiseModel(p1=p[0], p2=p[1], readout=p[2], trajectories=T, seed=seed)


def build(kind, n, trainable, readout, seed=0, net=None):
    """fp64 model on the CPU with two blocks per net (QuanONet: branch blocks of one sub-layer, trunk blocks of two; HEAQNN:
    `net`, default two blocks of two sub-layers); readout in 'Z', 'X', 'Y', 'diag'"""
    kw = dict(if_trainable_freq=trainable, scale_coeff=0.7, ham_bound=(-2.0, 3.0))
    if readout == 'diag':
        kw['ham_diag'] = np.random.default_rng(seed + 50).normal(size=1 << n)
    else:
        kw['ham_pauli'] = readout
    if kind == 'quanonet':
        m = H.quanonet(n, 3, 2, net or (2, 1, 2, 2), seed, **kw)
    else:
        m = H.heaqnn(n, 4, net or (2, 2), seed, **kw)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(seed + 7)
        for name, p in m.named_parameters():
            if name.endswith('freq.weights'):
                p.copy_(0.5 + torch.rand(p.shape, generator=gen, dtype=torch.float64))
    return m


def inputs(kind, rows, seed=1):
    rng = np.random.default_rng(seed)
    if kind == 'quanonet':
        return (rng.uniform(-1, 1, (rows, 3)), rng.uniform(0, 1, (rows, 2)))
    return (rng.uniform(-1, 1, (rows, 4)),)


def unbiased_case():
    """(model, inputs) of the unbiasedness check: n = 7, HEAQNN, one block, one row"""
    u = UNBIASED
    return build('heaqnn', u['n'], True, 'Z', seed=3, net=u['net']), inputs('heaqnn', 1, seed=11)


def within_sigmas(per_seed, exact, sigmas):
    """(ok, worst |mean - exact| / standard error): every component of the seeds' mean within `sigmas` standard errors"""
    per_seed = np.asarray(per_seed)
    mean = per_seed.mean(axis=0)
    se = per_seed.std(axis=0, ddof=1) / np.sqrt(per_seed.shape[0])
    dev = np.abs(mean - exact)
    # a component no draw reaches (the bias-free HEAQNN has none; kept for a zero spread) must be exact
    z = np.where(se > 0, dev / np.where(se > 0, se, 1.0), np.where(dev <= 1e-12, 0.0, np.inf))
    return bool(np.all(z <= sigmas)), float(z.max())


@pytest.mark.parametrize('kind', ['quanonet', 'heaqnn'])
@pytest.mark.parametrize('trainable', [True, False])
def test_noiseless_reference_is_the_ideal_oracle(kind, trainable):
    for n, readout in ((7, 'Z'), (7, 'X'), (7, 'Y'), (7, 'diag'), (8, 'Z')):
        m = build(kind, n, trainable, readout, seed=n)
        ins, y = inputs(kind, 3, seed=n), np.random.default_rng(n).normal(size=3)
        got, pred = TG.model_loss_grad(m, ins, y, 1.0 / 5, TG.TrajEngine(noise_model((0.0, 0.0, 0.0)), row0=4))
        ref, ref_pred = TG.model_loss_grad(m, ins, y, 1.0 / 5, None)
        assert got.shape == ref.shape == (sum(p.numel() for p in m.parameters()) + 2,)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(pred, ref_pred, rtol=0, atol=1e-12)


@pytest.mark.parametrize('kind,n,readout', [('heaqnn', 7, 'diag'), ('quanonet', 7, 'Y'), ('heaqnn', 8, 'X')])
def test_adjoint_and_central_difference_forms_agree(kind, n, readout):
    # (the diag case is kept small: every replay of the central differences mixes its 2^n table again, 4^n terms in Python)
    net = ((1, 1) if readout == 'diag' else (1, 2)) if kind == 'heaqnn' else (1, 1, 1, 1)
    m = build(kind, n, True, readout, seed=2, net=net)
    ins, y = inputs(kind, 2, seed=5), np.array([0.3, -0.4])
    settings = (((0.05, 0.1, 0.05), 0), ((1.0, 1.0, 0.0), 3_000_000_000))
    for p, row0 in settings[:1] if readout == 'diag' else settings:
        nz = noise_model(p, T=3, seed=9)
        adj, pa = TG.model_loss_grad(m, ins, y, 0.5, TG.TrajEngine(nz, row0))
        cd, pc = TG.model_loss_grad(m, ins, y, 0.5, TG.TrajEngine(nz, row0, form=TG.traj_grad_shift))
        np.testing.assert_allclose(adj, cd, rtol=0, atol=1e-12)
        np.testing.assert_allclose(pa, pc, rtol=0, atol=1e-13)
        assert np.abs(adj[:-2]).max() > 1e-3


def test_readout_table_is_the_oracles():
    from tests import noise_oracle as NO
    diag = np.random.default_rng(1).normal(size=128)
    for q in (0.0, 0.05, 0.5):
        np.testing.assert_allclose(TG.readout_table(diag, 7, q), NO.readout_diag(diag, 7, q), rtol=0, atol=1e-14)


def test_unbiasedness_of_the_reference():
    """the condition tests/test_noisy_traj_grad_abi.py holds the GPU to, with its seeds and T, on the reference alone"""
    u = UNBIASED
    m, ins = unbiased_case()
    exact = TG.dpred(m, ins, TG.ExactEngine(noise_model(u['rates'])))
    per_seed = [TG.dpred(m, ins, TG.TrajEngine(noise_model(u['rates'], T=u['T'], seed=s))) for s in u['seeds']]
    ok, worst = within_sigmas(per_seed, exact, u['sigmas'])
    spread = np.asarray(per_seed).std(axis=0, ddof=1)
    print(f"K={u['K']} T={u['T']}: worst deviation {worst:.2f} standard errors; per-seed spread {spread.min():.2e} .. "
          f"{spread.max():.2e}; max|exact|={np.abs(exact).max():.2e}")
    assert len(u['seeds']) == u['K'] and exact.shape == per_seed[0].shape
    assert ok, worst
    # the check has teeth: the ideal derivative (what a kernel that dropped the noise would return) fails it
    ideal = TG.dpred(m, ins, TG.TrajEngine(noise_model((0.0, 0.0, 0.0))))
    assert not within_sigmas(per_seed, ideal, u['sigmas'])[0]


@pytest.fixture(scope='module')
def lib():
    from quanonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'quanonet_amd', 'csrc'), '-j', '8'])
    return _lib.load()


def test_symbols_and_version(lib):
    from quanonet_amd import _lib
    assert lib.qhea_version() >= 580 and _lib.MIN_LIB_VERSION >= 580
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    for f in (_lib.model_loss_grad_noisy_wide, _lib.model_train_steps_noisy_wide, _lib.model_noisy_wide_grad_workspace_bytes):
        assert callable(f)
    from quanonet_amd.noise import noisy_loss_and_grad
    assert callable(noisy_loss_and_grad)


def _loss_grad(lib, d, batch, nz, ham_diag=None, row0=0):
    """the call with every array NULL: what the checks in front of the pointers return"""
    return lib.qhea_model_loss_grad_noisy_wide(None if d is None else ctypes.byref(d), row0, batch, None, None, None, None,
                                               ham_diag, None if nz is None else ctypes.byref(nz), 1.0, None, None, None, 0, None)


def _train_steps(lib, d, n_steps, nz, first_step=1):
    return lib.qhea_model_train_steps_noisy_wide(None if d is None else ctypes.byref(d), n_steps, None, None, None, None, None,
                                                 None, None if nz is None else ctypes.byref(nz), None, None, 0, None, None,
                                                 first_step, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, 0, None)


def test_abi_argument_checks_without_gpu(lib):
    from quanonet_amd import _lib
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, 8, (2, 1, 2, 2), 3, 2, True, 0.1, 0.0, 1.0)
    ok = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 40, 5)
    size = lambda dd, b, nz: lib.qhea_model_noisy_wide_grad_workspace_bytes(None if dd is None else ctypes.byref(dd), b,
                                                                            None if nz is None else ctypes.byref(nz))
    # the forward's tables, then (E + 3 n blk) doubles per (row, tile of 4) and per row: E = 32, blk = 6
    width, tiles = 32 + 3 * 8 * 6, 10
    fwd = lib.qhea_model_noisy_wide_workspace_bytes(ctypes.byref(d), 100, ctypes.byref(ok))
    assert size(d, 100, ok) >= fwd + 100 * tiles * width * 8 + 100 * width * 8 + 100 * 8
    assert size(d, 100, ok) < fwd + 100 * (tiles + 1) * width * 8 + 100 * tiles * 16 + 8192
    assert size(d, -1, ok) == 0 and size(None, 100, ok) == 0 and size(d, 100, None) == 0
    assert size(d, 100, _lib.NoiseParams(0.01, 0.02, 0.03, 10, 40, 5)) == 0              # shot mode has no gradient
    assert size(d, 100, _lib.NoiseParams(0.01, 0.02, 0.03, 0, 0, 5)) == 0
    d6 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 6, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    d10 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 10, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    assert size(d6, 100, ok) == 0 and size(d10, 100, ok) == 0
    bad_desc = _lib.make_model_desc(_lib.MODEL_QUANONET, 8, (2, 1, 2, 2), 3, 2, True, 0.1, 0.0, 1.0)
    bad_desc.n_qubits = 0
    bads = (_lib.NoiseParams(-0.1, 0, 0, 0, 1, 0), _lib.NoiseParams(0, 1.01, 0, 0, 1, 0), _lib.NoiseParams(0, 0, 2.0, 0, 1, 0),
            _lib.NoiseParams(0, 0, float('nan'), 0, 1, 0), _lib.NoiseParams(float('nan'), 0, 0, 0, 1, 0),
            _lib.NoiseParams(0, float('nan'), 0, 0, 1, 0), _lib.NoiseParams(0.01, 0.02, 0.03, 0, 0, 0),       # trajectories < 1
            _lib.NoiseParams(0.01, 0.02, 0.03, 7, 40, 0), _lib.NoiseParams(0.01, 0.02, 0.03, -1, 40, 0))      # shots
    for call in (_loss_grad, _train_steps):
        assert call(lib, bad_desc, 10, ok) == -1
        assert call(lib, None, 10, ok) == -1
        assert call(lib, d, 0, ok) == 0                                           # empty batch / no steps
        for bad in bads:
            assert call(lib, d, 10, bad) == -1
            assert call(lib, d6, 10, bad) == -1                                   # the noise setting is reported before the qubit count
            assert call(lib, d, 0, bad) == -1                                     # ... and before the empty batch
        assert call(lib, d, 10, None) == -1
        assert call(lib, d, -1, ok) == -1
        assert call(lib, d6, 10, ok) == -2 and call(lib, d10, 10, ok) == -2
        assert call(lib, d6, 0, ok) == -2                                         # the qubit range comes before the empty batch
        assert call(lib, d, 10, ok) == -1                                         # valid up to the NULL arrays
        # rates a density-matrix walk would refuse as ill-conditioned are fine here: no channel is inverted
        assert call(lib, d, 0, _lib.NoiseParams(1.0, 1.0, 0.5, 0, 3, 0)) == 0
    assert _loss_grad(lib, d, 10, ok, row0=-1) == -1
    assert _train_steps(lib, d, 3, ok, first_step=0) == -1
    assert _train_steps(lib, d, 0, ok, first_step=0) == -1
    dx = _lib.make_model_desc(_lib.MODEL_QUANONET, 7, (1, 1, 1, 1), 4, 1, True, 0.1, 0.0, 1.0)
    dx.ham_pauli = 1
    assert _loss_grad(lib, dx, 10, ok, ham_diag=ctypes.cast(ctypes.c_void_p(256), ctypes.POINTER(ctypes.c_double))) == -1


def test_train_steps_refusals_with_every_array_present(lib):
    """host arrays, no workspace: the checks read row_begin and nothing else, so nothing is launched"""
    from quanonet_amd import _lib
    from tests.test_noise_aware_abi import full_train_steps
    name = 'qhea_model_train_steps_noisy_wide'
    d = _lib.make_model_desc(_lib.MODEL_QUANONET, 7, (2, 1, 2, 1), 4, 1, True, 0.1, 0.0, 1.0)
    d6 = _lib.make_model_desc(_lib.MODEL_HEAQNN, 6, (2, 1), 3, 0, False, 0.1, 0.0, 1.0)
    ok, bad = _lib.NoiseParams(0.01, 0.02, 0.03, 0, 20, 0), _lib.NoiseParams(0, 1.01, 0, 0, 20, 0)
    table = [('first_step 0, no row_begin', dict(d=d, nz=ok, first_step=0, row_begin=False), -1),
             ('first_step 0, n = 6', dict(d=d6, nz=ok, first_step=0), -1),
             ('invalid rate, n = 6', dict(d=d6, nz=bad), -1),
             ('n = 6 alone', dict(d=d6, nz=ok), -2),
             ('no row_begin', dict(d=d, nz=ok, row_begin=False), -1),
             ('no workspace, a valid call of two steps', dict(d=d, nz=ok), -3)]
    for what, kw, want in table:
        assert full_train_steps(lib, name, **kw) == want, what
