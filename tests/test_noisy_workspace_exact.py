"""
The five noisy entry points on a workspace of exactly the size their *_workspace_bytes function names: the bytes after it
stay untouched, and the outputs are bitwise those of the same call on a roomy workspace.  Through ctypes, so that the buffer
and workspace_bytes are the test's own.  B = 5 rows; the trajectory calls run 150 trajectories per row (three tiles, the last
one partial), with and without ham_diag (the wide call's last region holds the table under the readout confusion).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

B, CANARY, FILL = 5, 4096, 0xA5
NETS = {'heaqnn': (3, 2), 'quanonet': (2, 1, 1, 2)}
NARROW = [(2, 'heaqnn'), (6, 'quanonet')]
WIDE = [(7, 'heaqnn'), (10, 'quanonet')]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _setup(n, kind, dev, with_diag):
    from quanonet_amd import _lib
    model = _lib.MODEL_QUANONET if kind == 'quanonet' else _lib.MODEL_HEAQNN
    desc = _lib.make_model_desc(model, n, NETS[kind], 3, 2, True, 0.1, 0.25, 0.5)
    P = _lib.model_param_count(desc)
    g = torch.Generator().manual_seed(100 * n + len(kind))
    r = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=g).to(dev)          # noqa: E731
    t = dict(branch=r(B, 3), trunk=r(B, 2), params=0.5 * r(P), y=r(B), diag=r(1 << n) if with_diag else None)
    return _lib, desc, P, t, _lib.NoiseParams(0.01, 0.02, 0.03, 0, 150, 11)


def _on_both_workspaces(dev, total, call):
    """call(ws pointer, ws bytes) -> output tensors; once on exactly `total` bytes followed by a canary, once with room to spare"""
    assert total > 0
    tight = torch.full((total + CANARY,), FILL, dtype=torch.uint8, device=dev)
    roomy = torch.full((2 * total + (1 << 20),), FILL, dtype=torch.uint8, device=dev)
    out_tight = call(ctypes.c_void_p(tight.data_ptr()), total)
    out_roomy = call(ctypes.c_void_p(roomy.data_ptr()), roomy.numel())
    torch.cuda.synchronize(dev)
    assert bool((tight[total:] == FILL).all()), "the call wrote past the size its workspace function names"
    for a, b in zip(out_tight, out_roomy):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        assert bool(torch.isfinite(a).all())


@pytest.mark.parametrize('with_diag', [False, True])
@pytest.mark.parametrize('n,kind,wide', [(n, k, False) for n, k in NARROW] + [(n, k, True) for n, k in WIDE])
def test_trajectory_calls(dev, n, kind, wide, with_diag):
    _lib, desc, P, t, noise = _setup(n, kind, dev, with_diag)
    lib = _lib.load()
    tag = 'noisy_wide' if wide else 'noisy'
    total = getattr(lib, f'qhea_model_{tag}_workspace_bytes')(ctypes.byref(desc), B, ctypes.byref(noise))

    def call(ws, ws_bytes):
        pred, se = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = getattr(lib, f'qhea_model_forward_{tag}')(ctypes.byref(desc), 7, B, _lib._ptr(t['branch']), _lib._ptr(t['trunk']),
                                                           _lib._ptr(t['params']), _lib._ptr(t['diag']), ctypes.byref(noise),
                                                           _lib._ptr(pred), _lib._ptr(se), ws, ws_bytes, _lib._stream(dev))
        assert rc == 0
        return pred, se
    _on_both_workspaces(dev, total, call)


@pytest.mark.parametrize('n,kind', NARROW)
def test_exact_forward(dev, n, kind):
    _lib, desc, P, t, noise = _setup(n, kind, dev, True)
    lib = _lib.load()
    total = lib.qhea_model_exact_noisy_workspace_bytes(ctypes.byref(desc), B)

    def call(ws, ws_bytes):
        pred, sd = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = lib.qhea_model_forward_noisy_exact(ctypes.byref(desc), B, _lib._ptr(t['branch']), _lib._ptr(t['trunk']),
                                                    _lib._ptr(t['params']), _lib._ptr(t['diag']), ctypes.byref(noise), _lib._ptr(pred),
                                                    _lib._ptr(sd), ws, ws_bytes, _lib._stream(dev))
        assert rc == 0
        return pred, sd
    _on_both_workspaces(dev, total, call)


@pytest.mark.parametrize('n,kind', NARROW)
def test_loss_grad(dev, n, kind):
    _lib, desc, P, t, noise = _setup(n, kind, dev, False)
    lib = _lib.load()
    total = lib.qhea_model_exact_noisy_grad_workspace_bytes(ctypes.byref(desc), B)

    def call(ws, ws_bytes):
        grad, pred = torch.empty(P + 2, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = lib.qhea_model_loss_grad_noisy_exact(ctypes.byref(desc), B, _lib._ptr(t['branch']), _lib._ptr(t['trunk']),
                                                      _lib._ptr(t['y']), _lib._ptr(t['params']), _lib._ptr(t['diag']),
                                                      ctypes.byref(noise), 1.0 / B, _lib._ptr(grad), _lib._ptr(pred), ws, ws_bytes,
                                                      _lib._stream(dev))
        assert rc == 0
        return grad, pred
    _on_both_workspaces(dev, total, call)


@pytest.mark.parametrize('n,kind', NARROW)
def test_train_steps(dev, n, kind):
    _lib, desc, P, t, noise = _setup(n, kind, dev, False)
    lib = _lib.load()
    bounds = [0, 1, 3, 5]                                          # three steps of 1, 2 and 2 rows: the size is the largest step's
    total = lib.qhea_model_exact_noisy_grad_workspace_bytes(ctypes.byref(desc), 2)
    rb = (ctypes.c_int64 * 4)(*bounds)
    ib = (ctypes.c_double * 3)(1.0, 0.5, 0.5)

    def call(ws, ws_bytes):
        params, m, v = t['params'].clone(), torch.zeros(P, dtype=torch.float64, device=dev), torch.zeros(P, dtype=torch.float64, device=dev)
        rows = torch.empty(3, P + 2, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = lib.qhea_model_train_steps_noisy_exact(ctypes.byref(desc), 3, rb, _lib._ptr(t['branch']), _lib._ptr(t['trunk']),
                                                        _lib._ptr(t['y']), _lib._ptr(params), None, ctypes.byref(noise), ib,
                                                        _lib._ptr(rows), P + 2, _lib._ptr(m), _lib._ptr(v), 1, 1e-2, 0.9, 0.999,
                                                        1e-8, 0.0, ws, ws_bytes, _lib._stream(dev))
        assert rc == 0
        return rows, params, m, v
    _on_both_workspaces(dev, total, call)
