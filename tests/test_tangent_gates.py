"""
Split-layout chains with the ansatz RY gates in tangent form (hea_zyz.hpp, SplitCoef): RY = c (I -/+ t X~), t = s / c, one
fma per gate on wires 0..3, the sub-layer's c0 c1 c2 c3 carried by wire 4's coefficients; hand-off slots of the LD = 2
reverse walk at a per-call offset (zquad_slot_offset).

Host: the tangent form against the standard form and a long-double reference, angles of exactly +-pi and pi - 1e-7 and the
record writer's clamp (|c| < 2^-100 -> +-2^-100) included.

GPU, n = 5, against the C oracle at the tolerances of test_hip_parity.py (1e-10: values, states, circuit gradients) and
test_snapshot_backward.py (1e-9: training steps against torch.optim.Adam):
* LD = 2 with 1, 3, 4, 6, 8 blocks (peeled blocks only, the unrolled body only, both, two passes of the hand-off ring) and
  LD = 1 with 2 and 5, through fwd_split_kernel, bwd_zquad_kernel (B = 3 and 2), bwd_zsnap_kernel and bwd_ztri_kernel<5, 2>
  (2 CUs + 1 samples: the smallest batch with more sample groups than CUs, odd);
* random angles, and a hard set: ansatz gates whose decomposition has |c| <= 1e-8 (one of them 0), encoding angles of
  exactly +-pi and pi - 1e-7; everything returned must be finite;
* training steps (model path): zsnap against oracle + Adam, zsnap against ztri2 at 1e-12 relative, bitwise repeatability,
  a multi-step call against single calls, an ensemble of two against the single-model runs (zquad).
"""
import copy

import numpy as np
import pytest
import torch

from oracle import hea_oracle as O
from oracle import c_oracle as C
from tests import helpers as H

TOL, TOL_STEPS = 1e-10, 1e-9
N = 5
SHAPES = [(2, 1), (2, 3), (2, 4), (2, 6), (2, 8), (1, 2), (1, 5)]        # (LD, nblocks)


# --------------------------------------------------------------------------------------------------
# host
# --------------------------------------------------------------------------------------------------
def _layer_standard(v, c, s, dtype):
    """RY on wires 0..3 of 32-vectors (rows of v; amplitude index bit q = wire q), the split chains' standard form"""
    v = v.astype(dtype)
    k = np.arange(32)
    for q in range(4):
        sign = np.where((k >> q) & 1, 1, -1).astype(dtype)
        v = c[:, q, None].astype(dtype) * v + sign * s[:, q, None].astype(dtype) * v[:, k ^ (1 << q)]
    return v


def _clamp(c):
    tiny = 2.0 ** -100
    return np.where(np.abs(c) < tiny, np.where(np.signbit(c), -tiny, tiny), c)


def _layer_tangent(v, c, s):
    """the same layer in tangent form: one multiply-add per gate, the product of the (clamped) cosines at the end"""
    k = np.arange(32)
    cc = _clamp(c)
    t = s / cc
    for q in range(4):
        sign = np.where((k >> q) & 1, 1.0, -1.0)
        v = v + (sign * t[:, q, None]) * v[:, k ^ (1 << q)]
    return ((cc[:, 0] * cc[:, 1]) * (cc[:, 2] * cc[:, 3]))[:, None] * v


def test_tangent_form_equals_standard_form_on_the_host():
    rng = np.random.default_rng(20)
    runs = 200
    v0 = rng.normal(size=(runs, 32))
    v0 /= np.linalg.norm(v0, axis=1, keepdims=True)
    a, b, ref = v0.copy(), v0.copy(), v0.astype(np.longdouble)
    special = np.array([np.pi, -np.pi, np.pi - 1e-7])
    for layer in range(180):
        th = rng.uniform(-np.pi, np.pi, (runs, 4))
        if layer % 7 == 3:
            th[np.arange(runs), rng.integers(0, 4, runs)] = special[np.arange(runs) % 3]
        c, s = np.cos(0.5 * th), np.sin(0.5 * th)
        if layer % 31 == 5:                                               # an exact zero: the clamp
            idx = rng.integers(0, 4, runs)
            c[np.arange(runs), idx], s[np.arange(runs), idx] = 0.0, 1.0
        a = _layer_standard(a, c, s, np.float64)
        b = _layer_tangent(b, c, s)
        ref = _layer_standard(ref, c, s, np.longdouble)
        assert np.isfinite(b).all(), layer
    ref = ref.astype(np.float64)
    assert np.abs(a - ref).max() < 1e-14                                  # the reference form itself: ~1e-15
    assert np.abs(b - a).max() < 1e-13 and np.abs(b - ref).max() < 1e-13, (np.abs(b - a).max(), np.abs(b - ref).max())


# --------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device('cuda:0')


def _t(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


def _gate_c(w3):
    """cos(theta / 2) of the ZYZ decomposition of RY(w3[2]) RZ(w3[1]) RY(w3[0]): |U_00|"""
    def ry(t):
        return np.array([[np.cos(t / 2), -np.sin(t / 2)], [np.sin(t / 2), np.cos(t / 2)]], dtype=complex)
    rz = np.diag([np.exp(-0.5j * w3[1]), np.exp(0.5j * w3[1])])
    return abs((ry(w3[2]) @ rz @ ry(w3[0]))[0, 0])


def _hard_ansatz(w, rng):
    """some gates of every other sub-layer with |c| <= 1e-8, one of them with c = 0; at least one wire below 4 and wire 4"""
    n_hard = 0
    for s in range(0, w.shape[0], 2):
        for q in {int(rng.integers(0, 4)), 4, int(rng.integers(0, 5))}:
            a = rng.uniform(-1.0, 1.0)
            w[s, :, q] = (a, 0.0, np.pi - 1e-8 - a)                      # RY(c) RY(a): cos((pi - 1e-8) / 2) = 5e-9
            n_hard += 1
    w[0, :, 1] = (0.5 * np.pi, 0.0, 0.5 * np.pi)                          # cos^2(pi/4) - sin^2(pi/4): 0 up to an ulp
    hard = [(s, q) for s in range(w.shape[0]) for q in range(5) if _gate_c(w[s, :, q]) <= 1e-8]
    assert len(hard) >= n_hard and (0, 1) in hard, hard
    return w


def _hard_encoding(x, rng):
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=max(3, flat.size // 6), replace=False)
    flat[idx] = np.resize([np.pi, np.pi - 1e-7, -np.pi], idx.size)
    assert (x == np.pi).any() and (x == np.pi - 1e-7).any()
    return x


_CASES = {}


def _case(ld, nblocks, B, hard):
    """inputs and oracle results of one shape, computed once and shared by the kernels' tests"""
    key = (ld, nblocks, B, hard)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * ld + 10 * nblocks + B + (7 if hard else 0))
        cfgs = [(N, ld)] * nblocks
        E, blk = O.circuit_sizes(N, cfgs)
        x = rng.uniform(-np.pi, np.pi, (B, E))
        w = rng.uniform(-np.pi, np.pi, (blk, 3, N))
        if hard:
            w, x = _hard_ansatz(w, rng), _hard_encoding(x, rng)
        g = rng.normal(size=B)
        off, co = O.ham_params(N, -2.0, 5.0)
        ro, rst = C.hea_forward(N, cfgs, x, w, off, co, return_state=True)
        _, rgx, rgw = C.hea_backward(N, cfgs, x, w, g, off, co)
        for a in (x, w, g, ro, rst, rgx, rgw):
            a.setflags(write=False)
        _CASES[key] = (cfgs, x, w, g, off, co, ro, rst, rgx, rgw)
    return _CASES[key]


def _check_circuit(dev, variant, ld, nblocks, B, hard, with_forward):
    from quanonet_amd import _lib
    cfgs, x, w, g, off, co, ro, rst, rgx, rgw = _case(ld, nblocks, B, hard)
    sh = _lib.CircuitShape(N, cfgs)
    xd, wd, gd = _t(x, dev), _t(w, dev), _t(g, dev)
    msg = f'{variant} ld={ld} nblocks={nblocks} B={B} hard={hard}'
    _lib.set_backward_variant(variant)
    try:
        if with_forward:
            out, st = _lib.hea_forward(sh, xd, wd, off, co, None, return_state=True)
            out, st = out.cpu().numpy(), st.cpu().numpy()
            assert np.isfinite(out).all() and np.isfinite(st).all(), msg
            np.testing.assert_allclose(out, ro, rtol=0, atol=TOL, err_msg=msg)
            np.testing.assert_allclose(st, rst, rtol=0, atol=TOL, err_msg=msg)
        gx, gw, out2 = _lib.hea_backward(sh, xd, wd, gd, off, co, None, state=None, want_out=True)
        torch.cuda.synchronize()
        gx, gw, out2 = gx.cpu().numpy(), gw.cpu().numpy(), out2.cpu().numpy()
    finally:
        _lib.set_backward_variant('auto')
        _lib.check_status(dev)
    assert np.isfinite(gx).all() and np.isfinite(gw).all() and np.isfinite(out2).all(), msg
    np.testing.assert_allclose(out2, ro, rtol=0, atol=TOL, err_msg=msg)
    np.testing.assert_allclose(gx, rgx, rtol=0, atol=TOL, err_msg=msg)
    np.testing.assert_allclose(gw, rgw, rtol=0, atol=TOL, err_msg=msg)


def _two_per_cu_batch(dev):
    """the smallest batch with more sample groups (two samples each) than CUs: AUTO takes bwd_zsnap_kernel from here on"""
    return 2 * torch.cuda.get_device_properties(dev).multi_processor_count + 1


@pytest.mark.gpu
@pytest.mark.parametrize('hard', [False, True])
@pytest.mark.parametrize('ld,nblocks', SHAPES)
def test_split_forward_and_quad_chain_backward(dev, ld, nblocks, hard):
    """fwd_split_kernel (forward of 3 samples) and bwd_zquad_kernel: B = 3 leaves the second group's second sample invalid"""
    for B in (3, 2):
        _check_circuit(dev, 'zquad', ld, nblocks, B, hard, with_forward=True)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['zsnap', 'ztri2'])
@pytest.mark.parametrize('hard', [False, True])
@pytest.mark.parametrize('ld,nblocks', SHAPES)
def test_snapshot_and_two_pipeline_backward(dev, ld, nblocks, hard, variant):
    """bwd_zsnap_kernel and bwd_ztri_kernel<5, 2>, whose split forward phase reads the same records and whose all-lane reverse
    walk reads the same (cos, sin) table"""
    _check_circuit(dev, variant, ld, nblocks, _two_per_cu_batch(dev), hard, with_forward=False)


@pytest.mark.gpu
@pytest.mark.parametrize('ld,nblocks', [(2, 3), (1, 5)])
def test_automatic_choice_at_the_two_per_cu_batch(dev, ld, nblocks):
    _check_circuit(dev, 'auto', ld, nblocks, _two_per_cu_batch(dev), False, with_forward=True)


# ---- training steps (model path)
def _model(net, seed, hard):
    m = H.quanonet(N, 4, 2, net, seed, scale_coeff=0.1, if_trainable_freq=True)
    if hard:
        rng = np.random.default_rng(seed)
        with torch.no_grad():
            w = m.quantum_layer.ansatz_weights
            shape = w.shape
            w.copy_(torch.from_numpy(_hard_ansatz(w.detach().numpy().reshape(-1, 3, N).copy(), rng).reshape(shape)))
    return m


def _steps(dev, variant, model, inputs, y, bounds, gbs, lr):
    from quanonet_amd import _lib
    _lib.set_backward_variant(variant)
    try:
        return H.run_single(dev, model.fused_desc(), model, inputs, y, bounds, gbs, lr)
    finally:
        _lib.set_backward_variant('auto')


@pytest.mark.gpu
@pytest.mark.parametrize('net,hard', [((6, 2, 2, 2), False), ((6, 2, 2, 2), True), ((3, 1, 2, 1), True), ((3, 2, 2, 2), False)])
def test_training_steps_match_oracle_and_agree_across_kernels(dev, net, hard):
    """cfg 2's net scaled down, three steps at the two-groups-per-CU batch: zsnap against the oracle + torch.optim.Adam, and
    against ztri2 (psi walked back in the all-lane layout) at 1e-12 relative"""
    B, steps, lr = _two_per_cu_batch(dev), 3, 1e-2
    bounds, gbs = H.schedule(B, steps)
    (inputs,), (y,) = H.member_data(1, bounds[-1], (4, 2), 77)
    model = _model(net, 3, hard)
    want_rows, want_params = H.oracle_adam(model, H.member_lossgrad('QuanONet', N, net), inputs, y, bounds, gbs, lr)
    p_snap, _, _, rows = _steps(dev, 'zsnap', model, inputs, y, bounds, gbs, lr)
    assert torch.isfinite(p_snap).all() and torch.isfinite(rows).all()
    np.testing.assert_allclose(rows.numpy(), want_rows, rtol=0, atol=TOL_STEPS)
    np.testing.assert_allclose(p_snap.numpy(), want_params, rtol=0, atol=TOL_STEPS)
    p_tri = _steps(dev, 'ztri2', model, inputs, y, bounds, gbs, lr)[0]
    assert float((p_snap - p_tri).abs().max()) <= 1e-12 * float(p_tri.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['zsnap', 'zquad'])
def test_steps_are_bitwise_repeatable_and_multi_step_equals_single_steps(dev, variant):
    """LD = 2 with 5 blocks (one peeled block in front of the unrolled body: a hand-off slot offset of 6)"""
    from quanonet_amd import _lib
    from quanonet_amd.solver import DataParallelTrainer
    net, steps, lr = (3, 2, 2, 2), 3, 1e-2
    B = _two_per_cu_batch(dev) if variant == 'zsnap' else 5
    rng = np.random.default_rng(8)
    branch, trunk, y = rng.normal(size=(steps * B, 4)), rng.uniform(size=(steps * B, 2)), rng.normal(scale=0.5, size=steps * B)
    bounds = [i * B for i in range(steps + 1)]
    model = _model(net, 5, False)
    _lib.set_backward_variant(variant)
    try:
        runs = []
        for rep in range(2):
            tr = DataParallelTrainer(copy.deepcopy(model).to(dev), lr=lr)
            rows = torch.zeros(steps, tr.numel + 2, dtype=torch.float64, device=dev)
            tr.train_steps([_t(branch, dev), _t(trunk, dev)], _t(y, dev).reshape(-1, 1), bounds, [B] * steps, rows)
            torch.cuda.synchronize()
            tr.check_status()
            runs.append((rows.cpu().numpy(), tr.pflat.cpu().numpy()))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        tr = DataParallelTrainer(copy.deepcopy(model).to(dev), lr=lr)
        single = []
        for i in range(steps):
            row = torch.zeros(tr.numel + 2, dtype=torch.float64, device=dev)
            sl = slice(i * B, (i + 1) * B)
            tr.train_step(_t(branch[sl], dev), _t(trunk[sl], dev), _t(y[sl], dev), global_batch=B, out=row)
            single.append(row.cpu().numpy())
        torch.cuda.synchronize()
        tr.check_status()
    finally:
        _lib.set_backward_variant('auto')
    assert np.isfinite(runs[0][0]).all() and np.isfinite(runs[0][1]).all()
    assert np.array_equal(np.stack(single), runs[0][0]) and np.array_equal(tr.pflat.cpu().numpy(), runs[0][1])


@pytest.mark.gpu
def test_ensemble_of_two_is_bitwise_the_single_model_runs(dev):
    """one member launch (bwd_zquad_kernel's member instantiation), as tests/test_ensemble.py asserts it for the headline net"""
    from quanonet_amd import _lib
    net, lr, R = (3, 2, 2, 2), 1e-2, 2
    bounds, gbs = H.schedule(6, 3, last=5)
    inputs, ys = H.member_data(R, bounds[-1], (4, 2), 31)
    models = [_model(net, seed, hard=bool(seed)) for seed in range(R)]
    desc = models[0].fused_desc()
    _lib.set_backward_variant('zquad')
    try:
        got = H.run_members(dev, 'ensemble', models, [lr] * R, inputs, ys, bounds, gbs, desc=desc)
        for m in range(R):
            want = H.run_single(dev, desc, models[m], inputs[m], ys[m], bounds, gbs, lr)
            for g, w, what in zip(got, want, ('params', 'exp_avg', 'exp_avg_sq', 'rows')):
                assert torch.isfinite(w).all(), (m, what)
                assert torch.equal(g[m], w), (m, what, float((g[m] - w).abs().max()))
    finally:
        _lib.set_backward_variant('auto')
