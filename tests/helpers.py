"""Shared helpers for the parity tests (test infrastructure; may import oracle/)."""
import json
import os
import numpy as np

from oracle import hea_oracle as O
from quanonet_amd.checkpoint import ms_to_pt_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_pt_params(fname, n, net_size):
    d = np.load(os.path.join(GOLDEN, fname), allow_pickle=False)
    return ms_to_pt_state({k: d[k] for k in d.files}, n, net_size)


def known_answers():
    with open(os.path.join(GOLDEN, 'known_answers.json')) as f:
        return json.load(f)


def notebook_inputs(npts, u0_fn):
    """visualization.ipynb cell 7: float32 grids, meshgrid 'xy', branch tiled."""
    x0 = np.linspace(0, 1, 100).astype(np.float32)
    x = np.linspace(0, 1, npts).astype(np.float32)
    X, YT = np.meshgrid(x, x)
    trunk = np.hstack((X.flatten()[:, None], YT.flatten()[:, None])).astype(np.float32)
    branch = np.tile(u0_fn(x0), (trunk.shape[0], 1)).astype(np.float32)
    return branch, trunk


U0 = {'sin2pi': lambda x: np.sin(2 * np.pi * x), 'sin4pi': lambda x: np.sin(4 * np.pi * x)}
PDE_CASES = [('K3', 'advection', 'sin2pi', 100), ('K4', 'advection', 'sin4pi', 100),
             ('K5', 'rdiffusion', 'sin2pi', 100), ('K6', 'rdiffusion', 'sin4pi', 100),
             ('K7', 'darcy', 'sin2pi', 25), ('K8', 'darcy', 'sin4pi', 25)]


def encode_quanonet(params, branch, trunk):
    """x[B,E] = cat(trunk_enc, branch_enc) in fp64 (models_pt.py:161-164)."""
    t = O.tiled_elementwise(trunk, params['trunk_freq.weights'], params['trunk_freq.bias'])
    b = O.tiled_elementwise(branch, params['branch_freq.weights'], params['branch_freq.bias'])
    return np.concatenate([t, b], axis=1)


def fmt1e(v):
    return f'{v:.1e}'


def golden_vectors():
    V = np.load(os.path.join(GOLDEN, 'hea_vectors.npz'), allow_pickle=False)
    names = sorted({k.split('.')[0] for k in V.files})
    out = {}
    for nm in names:
        out[nm] = dict(n=int(V[nm + '.n']), cfgs=[tuple(int(v) for v in r) for r in V[nm + '.cfgs']],
                       x=V[nm + '.x'], w=V[nm + '.w'], g=V[nm + '.g'], out=V[nm + '.out'],
                       grad_x=V[nm + '.grad_x'], grad_w=V[nm + '.grad_w'])
    return out


# --------------------------------------------------------------------------------------------------
# Test double for CPU-only host-logic tests: an nn.Module with the HEACircuitHIP surface whose
# arithmetic is the ORACLE.  Test infrastructure only -- the product never constructs it.
# --------------------------------------------------------------------------------------------------
def make_oracle_layer(n_wires, block_configs, ham_offset, ham_coeff):
    import torch
    import torch.nn as nn
    from oracle import c_oracle as C

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w):
            ctx.save_for_backward(x, w)
            out = C.hea_forward(n_wires, block_configs, x.detach().numpy(), w.detach().numpy(), ham_offset, ham_coeff)
            return torch.from_numpy(out)

        @staticmethod
        def backward(ctx, g):
            x, w = ctx.saved_tensors
            _, gx, gw = C.hea_backward(n_wires, block_configs, x.detach().numpy(), w.detach().numpy(),
                                       g.detach().numpy(), ham_offset, ham_coeff)
            return torch.from_numpy(gx), torch.from_numpy(gw)

    class OracleLayer(nn.Module):
        def __init__(self, init):
            super().__init__()
            self.ansatz_weights = nn.Parameter(init.clone())

        def forward(self, x):
            return _Fn.apply(x, self.ansatz_weights).unsqueeze(-1)

    return OracleLayer


def quanonet_with_oracle_layer(n, b_in, t_in, net, seed=0):
    """QuanONetPT (product class, host logic under test) with its quantum layer swapped for the oracle double."""
    import torch
    from quanonet_amd.models import QuanONetPT
    torch.manual_seed(seed)
    m = QuanONetPT(n, b_in, t_in, net, scale_coeff=0.1, if_trainable_freq=True)
    q = m.quantum_layer
    m.quantum_layer = make_oracle_layer(n, q.block_configs, q.ham_offset, q.ham_coeff)(q.ansatz_weights.data)
    return m


def swap_in_oracle_layer(model):
    """Replace a product module's HIP quantum layer by the oracle test double (same initial weights, same dtype)."""
    q = model.quantum_layer
    model.quantum_layer = make_oracle_layer(q.n_wires, q.block_configs, q.ham_offset, q.ham_coeff)(q.ansatz_weights.data)
    return model


def load_trajectory(name):
    """(case tuple, arrays) of tests/golden/ptsolver_trajectory.npz written by tests/golden/make_trajectory.py."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_trajectory', os.path.join(GOLDEN, 'make_trajectory.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    z = np.load(os.path.join(GOLDEN, 'ptsolver_trajectory.npz'), allow_pickle=False)
    arrs = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + '/')}
    return mod.CASES[name], arrs, mod.param_order


def trajectory_solver_inputs(name, prefix, **extra):
    """PTSolver config + DataManager-shaped data dict of one trajectory case (test rows = the first 40 train rows)."""
    (model_type, n, net, b_in, t_in, N, bs, epochs, lr, scale, trainable, seed), a, order = load_trajectory(name)
    cfg = {'model_type': model_type, 'operator': 'Trajectory', 'num_qubits': n, 'net_size': list(net),
           'scale_coeff': scale, 'if_trainable_freq': 'true' if trainable else 'false', 'learning_rate': lr,
           'batch_size': bs, 'num_epochs': epochs, 'prefix': prefix, 'run_id': name, 'trace_steps': True}
    cfg.update(extra)
    if model_type == 'QuanONet':
        data = {'train_branch_input': a['input0'], 'train_trunk_input': a['input1'], 'train_output': a['y'],
                'test_branch_input': a['input0'][:40], 'test_trunk_input': a['input1'][:40], 'test_output': a['y'][:40]}
    else:
        data = {'train_input': a['input0'], 'train_output': a['y'], 'test_input': a['input0'][:40],
                'test_output': a['y'][:40]}
    return cfg, data, a, order(model_type, trainable), seed


# --------------------------------------------------------------------------------------------------
# Kernels one call launches: stream capture through the HIP runtime's C API (relaxed mode); the graph is only read,
# never instantiated or replayed.  The call runs once uncaptured first, so every buffer and workspace then exists.
# --------------------------------------------------------------------------------------------------
HIP_CAPTURE_RELAXED = 2
HIP_GRAPH_NODE_KERNEL = 0


def hip_runtime():
    """the HIP runtime this process already uses (torch's), by its loaded path"""
    import ctypes
    import torch
    torch.cuda.init()
    with open('/proc/self/maps') as f:
        paths = {line.split()[-1] for line in f if 'libamdhip64' in line}
    assert paths, 'HIP runtime not loaded'
    hip = ctypes.CDLL(sorted(paths)[0])
    hip.hipStreamBeginCapture.argtypes = [ctypes.c_void_p, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    hip.hipGraphKernelNodeGetParams.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipKernelNameRefByPtr.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipKernelNameRefByPtr.restype = ctypes.c_char_p
    hip.hipGraphDestroy.argtypes = [ctypes.c_void_p]
    return hip


def _kernel_node_params_type():
    import ctypes

    class Dim3(ctypes.Structure):
        _fields_ = [('x', ctypes.c_uint32), ('y', ctypes.c_uint32), ('z', ctypes.c_uint32)]

    class KernelNodeParams(ctypes.Structure):            # hipKernelNodeParams (hip_runtime_api.h)
        _fields_ = [('blockDim', Dim3), ('extra', ctypes.c_void_p), ('func', ctypes.c_void_p), ('gridDim', Dim3),
                    ('kernelParams', ctypes.c_void_p), ('sharedMemBytes', ctypes.c_uint32)]
    return KernelNodeParams


def _captured_kernel_nodes(dev, call, visit):
    """visit(hip, node) for every kernel node of one captured call"""
    import ctypes
    import torch
    from quanonet_amd import _lib
    hip = hip_runtime()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        call()
        _lib.check_status(dev)
        s.synchronize()
        h = ctypes.c_void_p(s.cuda_stream)
        assert hip.hipStreamBeginCapture(h, HIP_CAPTURE_RELAXED) == 0
        try:
            call()
        finally:
            graph = ctypes.c_void_p()
            rc = hip.hipStreamEndCapture(h, ctypes.byref(graph))
        assert rc == 0 and graph.value
    try:
        n = ctypes.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
        nodes = (ctypes.c_void_p * n.value)()
        assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
        out = []
        for i in range(n.value):
            t = ctypes.c_int(-1)
            assert hip.hipGraphNodeGetType(nodes[i], ctypes.byref(t)) == 0
            if t.value == HIP_GRAPH_NODE_KERNEL:
                out.append(visit(hip, nodes[i], s))
        return out
    finally:
        assert hip.hipGraphDestroy(graph) == 0


def kernels_launched(dev, call):
    """number of kernel nodes of one captured call"""
    return len(_captured_kernel_nodes(dev, call, lambda hip, node, s: None))


def kernel_launches(dev, call):
    """[(mangled kernel name, gridDim, blockDim)] of one captured call, in node order; gridDim / blockDim as (x, y, z)"""
    import ctypes
    P = _kernel_node_params_type()

    def visit(hip, node, s):
        p = P()
        assert hip.hipGraphKernelNodeGetParams(node, ctypes.byref(p)) == 0
        name = hip.hipKernelNameRefByPtr(p.func, ctypes.c_void_p(s.cuda_stream))
        assert name, 'the HIP runtime has no name for a captured kernel'
        return (name.decode(), (p.gridDim.x, p.gridDim.y, p.gridDim.z), (p.blockDim.x, p.blockDim.y, p.blockDim.z))
    return _captured_kernel_nodes(dev, call, visit)


def mangled_is(name, ident, targs=None):
    """whether a mangled (Itanium) kernel name is the function `ident` -- its length-prefixed identifier, so that
    '10bwd_kernel' never matches '14lds_bwd_kernel' -- and, given targs, whether its template arguments begin with those
    integers ('Li5ELi2E' for <5, 2>)"""
    import re
    m = re.search(r'(?<![0-9])%d%s(I|E|v|P|R|S|$)' % (len(ident), re.escape(ident)), name)
    if not m:
        return False
    if targs is None:
        return True
    want = 'I' + ''.join(f'Li{int(v)}E' for v in targs)
    return name[m.end() - 1:].startswith(want)


def oracle_adam_loop(model_cpu, names, branch, trunk, y, bounds, gbs, n, net, lr, model_type='QuanONet', **kw):
    """Independent CPU loop: oracle loss/gradients (C engine) + torch.optim.Adam.  Returns (rows [steps, P+2], final flat
    params).  kw: read-out arguments of the oracle's loss (ham_bound, ham_pauli, ham_diag)."""
    import torch
    from oracle import c_oracle as C
    params = [p for _, p in model_cpu.named_parameters()]
    opt = torch.optim.Adam(params, lr=lr)
    rows = []
    for i in range(len(gbs)):
        lo, hi = bounds[i], bounds[i + 1]
        sd = {k: v.detach().numpy() for k, v in model_cpu.state_dict().items()}
        if model_type == 'QuanONet':
            loss, grads, _ = O.quanonet_loss_and_grads(sd, branch[lo:hi], trunk[lo:hi], y[lo:hi], n, net,
                                                       batch_total=gbs[i], engine=C, **kw)
        else:
            loss, grads, _ = O.heaqnn_loss_and_grads(sd, branch[lo:hi], y[lo:hi], n, net, batch_total=gbs[i], engine=C, **kw)
        flat = np.concatenate([np.asarray(grads[k], np.float64).reshape(-1) for k in names])
        rows.append(np.concatenate([flat, [loss * gbs[i], float((y[lo:hi] ** 2).sum())]]))
        opt.zero_grad()
        for k, p in zip(names, params):
            p.grad = torch.from_numpy(np.asarray(grads[k], np.float64).reshape(p.shape).copy())
        opt.step()
    return np.stack(rows), np.concatenate([p.detach().numpy().reshape(-1) for p in params])


# --------------------------------------------------------------------------------------------------
# Member launches (qhea_model_{ensemble,sweep,depth_sweep,qubit_sweep}_train_steps): models, data, the calls on fresh device
# tensors, each member's single-model run and the oracle + torch.optim.Adam loop of one member.
# --------------------------------------------------------------------------------------------------
def quanonet(n, b_in, t_in, net, seed, **kw):
    """QuanONetPT in fp64 with seeded frequency biases and bias 0.1 (seed + 1)"""
    import torch
    from quanonet_amd.models import QuanONetPT
    torch.manual_seed(seed)
    m = QuanONetPT(n, b_in, t_in, net, **kw).double()
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        if hasattr(m, 'branch_freq') and hasattr(m.branch_freq, 'bias'):
            m.branch_freq.bias.copy_(torch.from_numpy(rng.normal(scale=0.3, size=m.branch_freq.bias.shape)))
            m.trunk_freq.bias.copy_(torch.from_numpy(rng.normal(scale=0.3, size=m.trunk_freq.bias.shape)))
        m.bias.fill_(0.1 * (seed + 1))
    return m


def heaqnn(n, x_in, net, seed, **kw):
    import torch
    from quanonet_amd.models import HEAQNNPT
    torch.manual_seed(seed)
    kw.setdefault('scale_coeff', 0.1)
    kw.setdefault('if_trainable_freq', True)
    return HEAQNNPT(n, x_in, net, **kw).double()


def flat(m):
    import torch
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()])


def schedule(batch, steps=3, last=None):
    """(row bounds, batch sizes) of `steps` steps of `batch` rows, the last one of `last` rows if given"""
    sizes = [batch] * (steps - 1) + [last if last is not None else batch]
    bounds = [0]
    for s in sizes:
        bounds.append(bounds[-1] + s)
    return bounds, sizes


def member_data(R, n_rows, widths, seed):
    """R members' inputs ([normal, uniform, ...] of the given widths) and targets"""
    rng = np.random.default_rng(seed)
    inputs = [[rng.normal(size=(n_rows, w)) if k == 0 else rng.uniform(size=(n_rows, w)) for k, w in enumerate(widths)]
              for _ in range(R)]
    ys = [rng.normal(scale=0.5, size=n_rows) for _ in range(R)]
    return inputs, ys


def member_hp(desc, lr):
    from quanonet_amd import _lib
    return _lib.member_hparams(desc.scale_coeff, desc.ham_offset, desc.ham_coeff, lr, desc.ham_pauli)


MEMBER_ENTRIES = ('ensemble', 'sweep', 'depth', 'qubit')


def member_call(dev, entry, models, lrs, inputs, ys, bounds, gbs, ham_diag=None, sentinel=0.0, rows_sentinel=0.0, rows_extra=0,
                desc=None):
    """(call, (params, exp_avg, exp_avg_sq, rows)): one member entry point's call on fresh device tensors; the call may be run
    or captured.  entry: 'ensemble' (models[0]'s descriptor, lrs[0], ham_diag one spectrum), 'sweep' (models[0]'s shape, each
    member's read-out, scale and lr; ham_diag [R, 2^n]), 'depth' or 'qubit' (each member's descriptor; ham_diag: a spectrum per
    member, padded with `sentinel` to the widest).  params / moments [R, Pmax], `sentinel` beyond each member's vector; rows
    [R, steps, Pmax + 2 + rows_extra] filled with rows_sentinel.  desc: the ensemble / sweep descriptor if not models[0]'s."""
    import torch
    from quanonet_amd import _lib
    assert entry in MEMBER_ENTRIES, entry
    descs = [m.fused_desc() for m in models]
    d0 = desc if desc is not None else descs[0]
    R = len(models)
    flats = [flat(m) for m in models]
    P = max(f.numel() for f in flats)
    params = torch.full((R, P), sentinel, dtype=torch.float64)
    m_, v_ = params.clone(), params.clone()
    for i, f in enumerate(flats):
        params[i, :f.numel()] = f
        m_[i, :f.numel()] = 0.0
        v_[i, :f.numel()] = 0.0
    params, m_, v_ = params.to(dev), m_.to(dev), v_.to(dev)
    rows = torch.full((R, len(gbs), P + 2 + rows_extra), rows_sentinel, dtype=torch.float64, device=dev)
    ins = [torch.from_numpy(np.stack([inp[k] for inp in inputs])).to(dev) for k in range(len(inputs[0]))]
    y = torch.from_numpy(np.stack(ys)).to(dev)
    b, t = ins[0], (ins[1] if len(ins) > 1 else None)
    hd = None
    if torch.is_tensor(ham_diag):
        hd = ham_diag.to(dev)
    elif ham_diag is not None and entry == 'ensemble':
        hd = torch.from_numpy(np.asarray(ham_diag, np.float64)).to(dev)
    elif ham_diag is not None:
        width = max(len(h) for h in ham_diag)
        hd = torch.full((R, width), sentinel, dtype=torch.float64)
        for i, h in enumerate(ham_diag):
            hd[i, :len(h)] = torch.from_numpy(np.asarray(h, np.float64))
        hd = hd.to(dev)
    hps = [member_hp(d, lr) for d, lr in zip(descs, lrs)]
    if entry == 'ensemble':
        def call():
            _lib.model_ensemble_train_steps(d0, bounds, gbs, b, t, y, params, rows, m_, v_, 1, lrs[0], 0.9, 0.999, 1e-8, 0.0,
                                            ham_diag=hd)
    elif entry == 'sweep':
        def call():
            _lib.model_sweep_train_steps(d0, hps, bounds, gbs, b, t, y, params, rows, m_, v_, 1, 0.9, 0.999, 1e-8, 0.0,
                                         ham_diag=hd)
    else:
        fn = _lib.model_depth_sweep_train_steps if entry == 'depth' else _lib.model_qubit_sweep_train_steps

        def call():
            fn(descs, hps, bounds, gbs, b, t, y, params, rows, m_, v_, 1, 0.9, 0.999, 1e-8, 0.0, ham_diag=hd)
    return call, (params, m_, v_, rows)


def run_members(dev, entry, models, lrs, inputs, ys, bounds, gbs, ham_diag=None, **kw):
    """member_call run once: (params, exp_avg, exp_avg_sq, rows) on the CPU"""
    from quanonet_amd import _lib
    call, out = member_call(dev, entry, models, lrs, inputs, ys, bounds, gbs, ham_diag=ham_diag, **kw)
    call()
    _lib.check_status(dev)
    return tuple(o.cpu() for o in out)


def run_single(dev, desc, model, inputs, y, bounds, gbs, lr, ham_diag=None):
    """model_train_steps of one model: (params, exp_avg, exp_avg_sq, rows) on the CPU"""
    import torch
    from quanonet_amd import _lib
    params = flat(model).to(dev).contiguous()
    P = params.numel()
    m_, v_ = torch.zeros_like(params), torch.zeros_like(params)
    rows = torch.zeros(len(gbs), P + 2, dtype=torch.float64, device=dev)
    ins = [torch.from_numpy(t).to(dev) for t in inputs]
    _lib.model_train_steps(desc, bounds, gbs, ins[0], ins[1] if len(ins) > 1 else None, torch.from_numpy(y).to(dev), params,
                           rows, m_, v_, 1, lr, 0.9, 0.999, 1e-8, 0.0, ham_diag=ham_diag)
    _lib.check_status(dev)
    return params.cpu(), m_.cpu(), v_.cpu(), rows.cpu()


def oracle_adam(model, lossgrad, inputs, y, bounds, gbs, lr):
    """oracle loss / gradients (lossgrad(state dict, inputs, y, batch_total) -> (loss, grads)) + torch.optim.Adam on a CPU copy:
    (rows [steps, P+2], final flat parameters)"""
    return oracle_adam_state(model, lossgrad, inputs, y, bounds, gbs, lr)[:2]


def oracle_adam_state(model, lossgrad, inputs, y, bounds, gbs, lr):
    """oracle_adam, also returning torch.optim.Adam's exp_avg / exp_avg_sq flattened in parameter order"""
    import copy
    import torch
    cpu = copy.deepcopy(model).cpu()
    names = [k for k, _ in cpu.named_parameters()]
    params = [p for _, p in cpu.named_parameters()]
    opt = torch.optim.Adam(params, lr=lr)
    rows = []
    for i, gb in enumerate(gbs):
        lo, hi = bounds[i], bounds[i + 1]
        sd = {k: v.detach().numpy() for k, v in cpu.state_dict().items()}
        loss, grads = lossgrad(sd, [t[lo:hi] for t in inputs], y[lo:hi], gb)
        flat_g = np.concatenate([np.asarray(grads[k], np.float64).reshape(-1) for k in names])
        rows.append(np.concatenate([flat_g, [loss * gb, float((y[lo:hi] ** 2).sum())]]))
        for k, p in zip(names, params):
            p.grad = torch.from_numpy(np.asarray(grads[k], np.float64).reshape(p.shape).copy())
        opt.step()
    st = [opt.state[p] for p in params]
    m1 = np.concatenate([s['exp_avg'].numpy().reshape(-1) for s in st])
    m2 = np.concatenate([s['exp_avg_sq'].numpy().reshape(-1) for s in st])
    return np.stack(rows), np.concatenate([p.detach().numpy().reshape(-1) for p in params]), m1, m2


def member_lossgrad(kind, n, net, ham_bound=(-5.0, 5.0), ham_pauli='Z', ham_diag=None, scale_coeff=None):
    """oracle loss / gradients of one member (C engine) for oracle_adam: kind 'QuanONet' or 'HEAQNN'"""
    from oracle import c_oracle as C

    def f(sd, ins, y, gb):
        kw = dict(ham_bound=ham_bound, batch_total=gb, ham_pauli=ham_pauli, ham_diag=ham_diag, scale_coeff=scale_coeff, engine=C)
        if kind == 'QuanONet':
            loss, grads, _ = O.quanonet_loss_and_grads(sd, ins[0], ins[1], y, n, net, **kw)
        else:
            loss, grads, _ = O.heaqnn_loss_and_grads(sd, ins[0], y, n, net, **kw)
        return loss, grads
    return f


def assert_checkpoints_bitwise(dir_a, dir_b, what=None):
    """best_model.npz and final.npz of two runs (their output directories) hold the same arrays, bit for bit"""
    for f in ('best_model.npz', 'final.npz'):
        with np.load(os.path.join(dir_a, f)) as a, np.load(os.path.join(dir_b, f)) as b:
            assert sorted(a.files) == sorted(b.files), (what, f)
            for k in a.files:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, f, k)
