"""
Encoding (RX-chunk) gradients of the split-layout pipelines' sigma walk (``zsigma_walk``: ``bwd_zsnap_kernel`` and
``bwd_zquad_kernel``), which are formed from per-sample butterfly sums of the chunk sub-layer's products.

* circuit-level ``grad_x`` and ``grad_w`` of both forced variants against the C oracle at 1e-9, block-unrolled n = 5 shapes
  with one and two sub-layers per block, at B = 1024, 1000, 512, 100 and 37 (a last sample group with one sample);
* both variants against ``ztri2`` (the all-lane pipeline with its own inline sigma walk) to 1e-12 relative;
* two runs of each variant are bitwise identical;
* the headline model's training rows (parameter gradients, through grad_x for the trainable frequencies) under both variants
  against the oracle at 1e-9.
"""
import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from oracle import c_oracle as C
from tests.test_snapshot_backward import _data, _headline_model, _oracle_adam, _train

pytestmark = pytest.mark.gpu
N = 5
SHAPES = {'ld2': [(N, 2)] * 12, 'ld1': [(N, 1)] * 9}
BATCHES = [1024, 1000, 512, 100, 37]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _backward(variant, cfgs, x, w, g, off, co, dev):
    from quanonet_amd import _lib
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    _lib.set_backward_variant(variant)
    try:
        gx, gw = _lib.hea_backward(_lib.CircuitShape(N, cfgs), t(x), t(w), t(g), off, co)
        torch.cuda.synchronize()
        _lib.check_status(dev)
    finally:
        _lib.set_backward_variant('auto')
    return gx.cpu().numpy(), gw.cpu().numpy()


def _case(shape, B):
    cfgs = SHAPES[shape]
    rng = np.random.default_rng(7000 + B + 31 * len(cfgs))
    E, blk = O.circuit_sizes(N, cfgs)
    x = rng.uniform(-np.pi, np.pi, (B, E))
    w = rng.uniform(-np.pi, np.pi, (blk, 3, N))
    g = rng.normal(size=B)
    off, co = O.ham_params(N, -2.0, 5.0)
    return cfgs, x, w, g, off, co


@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('B', BATCHES)
def test_chunk_gradients_match_oracle_ztri2_and_repeat(dev, shape, B):
    cfgs, x, w, g, off, co = _case(shape, B)
    _, rgx, rgw = C.hea_backward(N, cfgs, x, w, g, off, co)
    tgx, tgw = _backward('ztri2', cfgs, x, w, g, off, co, dev)
    for variant in ('zsnap', 'zquad'):
        gx, gw = _backward(variant, cfgs, x, w, g, off, co, dev)
        np.testing.assert_allclose(gx, rgx, rtol=0, atol=1e-9, err_msg=f'{variant} grad_x')
        np.testing.assert_allclose(gw, rgw, rtol=0, atol=1e-9, err_msg=f'{variant} grad_w')
        assert np.abs(gx - tgx).max() <= 1e-12 * np.abs(tgx).max(), (variant, 'grad_x vs ztri2')
        assert np.abs(gw - tgw).max() <= 1e-12 * np.abs(tgw).max(), (variant, 'grad_w vs ztri2')
        gx2, gw2 = _backward(variant, cfgs, x, w, g, off, co, dev)
        assert np.array_equal(gx, gx2) and np.array_equal(gw, gw2), (variant, 'not bitwise reproducible')


@pytest.mark.parametrize('batch', [1024, 100])
def test_headline_rows_match_oracle(dev, batch):
    steps, lr = 2, 1e-3
    rng = np.random.default_rng(1300 + batch)
    branch, trunk, y = _data(rng, steps * batch)
    bounds = [i * batch for i in range(steps + 1)]
    gbs = [batch] * steps
    model = _headline_model(rng, seed=3)
    want_rows, want_params = _oracle_adam(model, branch, trunk, y, bounds, gbs, N, (40, 2, 20, 2), lr)
    for variant in ('zsnap', 'zquad'):
        got_rows, got_params = _train(model, dev, variant, branch, trunk, y, bounds, gbs, lr)
        np.testing.assert_allclose(got_rows, want_rows, rtol=0, atol=1e-9, err_msg=variant)
        np.testing.assert_allclose(got_params, want_params, rtol=0, atol=1e-9, err_msg=variant)
