"""
Error budgets: one table of cases and one budget rule for every kernel family, against the long-double oracle
(oracle/ld_oracle.py).  Test infrastructure; importing it needs no GPU.  tests/test_precision_oracle.py (CPU) checks the
references and the inputs, tests/test_precision_budget.py (GPU) the kernels, scripts/precision_budget.py records the figures.

Budget of a quantity q (out, state, grad_x, grad_w; at model level the gradient row, the sse and the predictions):

    e_ref(q)  = max( max|q_C64 - q_ld| , max|q_numpy64 - q_ld| )     the two independent fp64 oracles' own error on these inputs
    budget(q) = FACTOR * max( e_ref(q) , 2^-53 * max|q_ld| )

e_ref comes from the references alone, at run time; no number of the code under test enters it.
"""
from collections import namedtuple

import numpy as np

from oracle import hea_oracle as O
from oracle import c_oracle as C
from oracle import ld_oracle as L
from tests.test_dispatch_regimes import BWD_KERNELS, FWD_KERNELS, CUS_NOMINAL, expected, lane_bits
from tests.test_tangent_gates import _hard_ansatz, _hard_encoding

# Why 32.  Two correct fp64 evaluations of the same circuit (the C and the numpy oracle) differ from the long-double value by
# amounts up to 5 times apart on the shapes below: rounding luck of the summation order, nothing else.  The differences the
# project has recorded for its kernels against the fp64 oracle (before this table existed: 3e-12 for
# gradients over 1024 samples, 1e-13 for outputs) are 12 to 14 times the oracles' own error at those shapes.  32 is the next
# power of two above twice that: room for a correct kernel that sums in another order and normalises through rsqrt, none for
# one that loses a decimal digit more.  One constant for every case and quantity; it is not tuned per case.
FACTOR = 32
ULP = 2.0 ** -53
HAM_BOUND = (-5.0, 5.0)                      # read-out bound of every case: outputs in [-5, 5]

INPUT_SETS = ('random', 'hard', 'wide')
# wide: every seventh encoding angle cycles through these.  fast_sincos (hea_sincos.hpp) hands |x| >= 1e5 to the device
# library's sincos, the kernels call it on the HALF angle: the branch flips at |angle| = 2e5, and these sit on both sides.
WIDE_SPECIAL = (1.99999e5, -1.99999e5, 2.5e5, -2.5e5)

Case = namedtuple('Case', 'id n cfgs batch inputs readout variant fwd bwd')
# batch: cus -> B.  readout: 'Z', 'X', 'Y' or 'diag'.  variant: qhea_set_backward_variant's name.  fwd / bwd: (kernel identifier,
# leading integer template arguments or None) the case must launch.


def _groups_batch(n, groups):
    """the smallest batch with that many sample groups"""
    return (groups - 1) * (64 >> lane_bits(n)) + 1


def _ragged(n):
    return [(n, 1), (n - 1, 2), (n, 1), (n + 1, 1)]                       # tests/test_dispatch_regimes.py: not block-unrolled


def _circuit_cases():
    out = []

    def add(name, n, cfgs, batch, sets, readout='Z', variant='auto', fwd=None, bwd=None):
        for s in sets:
            out.append(Case(f'{name}-{s}', n, cfgs, batch, s, readout, variant, fwd, bwd))

    every, rnd = INPUT_SETS, ('random',)
    split, quad = ('fwd_split_kernel', None), ('bwd_zquad_kernel', None)
    # n = 5, blocks (5, LD): the split-layout families
    add('q5-zquad-ld2x8', 5, [(5, 2)] * 8, lambda c: 3, every, fwd=split, bwd=quad)
    add('q5-zquad-ld1x5', 5, [(5, 1)] * 5, lambda c: 3, every, fwd=split, bwd=quad)
    two = lambda c: 2 * c + 1                                             # more sample groups than CUs, odd
    add('q5-zsnap-ld2x8', 5, [(5, 2)] * 8, two, every, fwd=split, bwd=('bwd_zsnap_kernel', None))
    add('q5-zsnap-ld2x30', 5, [(5, 2)] * 30, two, rnd, fwd=split, bwd=('bwd_zsnap_kernel', None))       # the headline depth
    add('q5-ztri2-ld2x8', 5, [(5, 2)] * 8, two, every, variant='ztri2', fwd=split, bwd=('bwd_ztri_kernel', (5, 2)))
    add('q5-ztri2-ld2x30', 5, [(5, 2)] * 30, two, rnd, variant='ztri2', fwd=split, bwd=('bwd_ztri_kernel', (5, 2)))
    # one pipeline per workgroup, forced; the X read-out takes the private-ring forward, a diagonal Hamiltonian the split one
    three = lambda c: 3 * c + 1
    add('q5-ztri1-X', 5, [(5, 2)] * 8, three, every, readout='X', variant='ztri', fwd=('fwd_zyz_kernel', None),
        bwd=('bwd_ztri_kernel', (5, 1)))
    add('q5-ztri1-diag', 5, [(5, 2)] * 8, three, every, readout='diag', variant='ztri', fwd=split,
        bwd=('bwd_ztri_kernel', (5, 1)))
    # one ring per workgroup and the one-wave backward: the smallest batch with 8 groups > 6 SIMDs (where AUTO leaves the
    # pipelines); forced, because AUTO's forward shares the ring only beyond one wave per SIMD
    add('q5-zpacked-ld2x4', 5, [(5, 2)] * 4, lambda c: _groups_batch(5, 6 * 4 * c // 8 + 1), every, variant='zpacked',
        fwd=('fwd_zshared_kernel', None), bwd=('bwd_zpacked_kernel', None))
    # first generation at n = 5, forced
    first = ('fwd_kernel', None)
    add('q5-tri', 5, [(5, 2)] * 3, lambda c: 7, every, variant='tri', fwd=first, bwd=('bwd_tri_kernel', None))
    add('q5-pair', 5, [(5, 2)] * 3, lambda c: 7, rnd, variant='pair', fwd=first, bwd=('bwd_pair_kernel', None))
    add('q5-packed', 5, [(5, 2)] * 3, lambda c: 7, rnd, variant='packed', fwd=first, bwd=('bwd_kernel', (5,)))
    # n = 2, 3, 4, ragged: the generic ZYZ walk (the hard set needs five wires); and a (cos, sin) table that does not fit
    for n in (2, 3, 4):
        add(f'q{n}-ragged', n, _ragged(n), lambda c: 40, ('random', 'wide') if n == 3 else rnd,
            fwd=('fwd_zyz_kernel', None), bwd=('bwd_ztri_kernel', (n, 1)))
    add('q2-E78', 2, [(2, 1)] * 39, lambda c: 40, rnd, fwd=first, bwd=('bwd_tri_kernel', None))
    # n = 6 .. 9: first generation, one sample per wave; n = 8 in the dense build (more waves than SIMDs)
    add('q6', 6, [(6, 1)] * 4, lambda c: 33, every, fwd=first, bwd=('bwd_kernel', (6,)))
    add('q9', 9, [(9, 1)] * 3, lambda c: 9, rnd, fwd=first, bwd=('bwd_kernel', (9,)))
    add('q8-dense', 8, [(8, 1)] * 3, lambda c: 4 * c + 1, rnd, fwd=first, bwd=('bwd_kernel', (8, 2)))
    # n = 10, 12: workgroup-resident
    lds = dict(fwd=('lds_fwd_kernel', None), bwd=('lds_bwd_kernel', None))
    add('q10', 10, [(10, 1)] * 2, lambda c: 5, every, **lds)
    add('q12', 12, [(12, 1)] * 2, lambda c: 2, rnd, **lds)
    return out


CIRCUIT_CASES = _circuit_cases()

ModelCase = namedtuple('ModelCase', 'id kind n net b_in t_in batch trainable reach scale')
# reach: None, or the magnitude the branch frequency layer's outputs are scaled to (through the branch inputs).  scale: the
# models' scale_coeff (the initial frequency weights, or the fixed scale).
# Why the +-1e3 case has frequency weights of 8 and not 0.1.  At |angle| = 1e3 the encoded angle in * w + b is itself rounded
# to 2^-43 = 1.1e-13 in fp64, in any correct evaluation; the row's entries d loss / d branch_freq.weights = sum_b grad_x[b] in[b]
# carry that rounding times |in| = 1e3 / |w|.  With w = 0.1 (|in| up to 5.6e3) both fp64 oracles are 4.2e-12 off the long-double
# row -- 7.5e-16 per unit of |in| --, which no kernel could undercut and which puts 32 x e_ref above the 1e-11 every budget is
# held to (tests/test_precision_oracle.py).  That cap admits |in| <= 1e-11 / 32 / 7.5e-16 = 415, i.e. |w| >= 2.4; 8 is the next
# power of two with a margin of two.  The angles the kernels see reach +-1e3 all the same.
MODEL_CASES = [
    ModelCase('quanonet-q5-trainable', 'QuanONet', 5, (3, 2, 2, 2), 6, 2, 53, True, None, 0.1),
    ModelCase('quanonet-q5-trainable-1e3', 'QuanONet', 5, (3, 2, 2, 2), 6, 2, 53, True, 1e3, 8.0),
    ModelCase('quanonet-q5-fixed', 'QuanONet', 5, (3, 2, 2, 2), 6, 2, 53, False, None, 0.1),
    ModelCase('heaqnn-q4', 'HEAQNN', 4, (3, 2), 6, 0, 53, True, None, 0.1),
    ModelCase('quanonet-q10', 'QuanONet', 10, (2, 1, 2, 1), 6, 2, 5, True, None, 0.1),
]

# case id -> seed, where the default (the case's position in its table) breaks the condition on the inputs: on a single
# number like the sse one oracle can land on the long-double value by luck
SEEDS = {'quanonet-q5-fixed': 7}


def _seed(case, table):
    base = 100 if table is CIRCUIT_CASES else 0          # (a model's bias is 0.1 x (seed + 1): tests/helpers.py quanonet)
    return SEEDS.get(case.id, base + [c.id for c in table].index(case.id))


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------------------------------------------------
def circuit_inputs(case, B):
    """(x[B,E], w[blk,3,n], g[B], offset, coeff, ham_diag or None, pauli letter), seeded by the case"""
    n = case.n
    E, blk = O.circuit_sizes(n, case.cfgs)
    rng = np.random.default_rng(_seed(case, CIRCUIT_CASES))
    x = rng.uniform(-np.pi, np.pi, (B, E))
    w = rng.uniform(-np.pi, np.pi, (blk, 3, n))
    if case.inputs == 'hard':
        w, x = _hard_ansatz(w, rng), _hard_encoding(x, rng)
    elif case.inputs == 'wide':
        x = rng.uniform(-1e3, 1e3, (B, E))
        flat = x.reshape(-1)
        flat[::7] = np.resize(WIDE_SPECIAL, flat[::7].size)
    g = rng.normal(size=B)
    off, co = O.ham_params(n, *HAM_BOUND)
    diag = np.sort(rng.uniform(*HAM_BOUND, size=1 << n)) if case.readout == 'diag' else None
    return x, w, g, off, co, diag, ('Z' if case.readout == 'diag' else case.readout)


Reference = namedtuple('Reference', 'inputs ld e_c e_np')      # ld: {quantity: (hi, lo)}; e_c / e_np: {quantity: max abs error}
_REFS = {}


def _maxabs(a):
    return float(np.abs(a).max()) if np.size(a) else 0.0


def circuit_reference(case, B):
    """the long-double results of one case and each fp64 oracle's error against them, computed once"""
    key = (case.id, B)
    if key not in _REFS:
        inputs = circuit_inputs(case, B)
        x, w, g, off, co, diag, pauli = inputs
        n, cfgs = case.n, case.cfgs
        ld = {}
        ld['out'], ld['state'] = L.hea_forward(n, cfgs, x, w, off, co, diag, return_state=True, ham_pauli=pauli)
        _, ld['grad_x'], ld['grad_w'] = L.hea_backward(n, cfgs, x, w, g, off, co, diag, ham_pauli=pauli)
        c_out, c_st = C.hea_forward(n, cfgs, x, w, off, co, diag, return_state=True, ham_pauli=pauli)
        _, c_gx, c_gw = C.hea_backward(n, cfgs, x, w, g, off, co, diag, ham_pauli=pauli)
        psi = O.hea_state(n, cfgs, x, w)
        n_out, n_gx, n_gw = O.hea_backward(n, cfgs, x, w, g, off, co, diag, ham_pauli=pauli)
        n_st = np.stack([psi.real, psi.imag], axis=-1)
        e_c = {q: _maxabs(L.err(v, ld[q])) for q, v in (('out', c_out), ('state', c_st), ('grad_x', c_gx), ('grad_w', c_gw))}
        e_np = {q: _maxabs(L.err(v, ld[q])) for q, v in (('out', n_out), ('state', n_st), ('grad_x', n_gx), ('grad_w', n_gw))}
        for a in inputs[:3] + tuple(v for pair in ld.values() for v in pair):
            a.setflags(write=False)
        _REFS[key] = Reference(inputs, ld, e_c, e_np)
    return _REFS[key]


def e_ref(ref, q):
    return max(ref.e_c[q], ref.e_np[q])


def budget(ref, q):
    return FACTOR * max(e_ref(ref, q), ULP * _maxabs(ref.ld[q][0]))


def model_of(case):
    """the case's model (fp64, on the CPU), its block list and its data (branch, trunk or None, y)"""
    from tests import helpers as H
    seed = _seed(case, MODEL_CASES)
    if case.kind == 'QuanONet':
        m = H.quanonet(case.n, case.b_in, case.t_in, case.net, seed, scale_coeff=case.scale, if_trainable_freq=case.trainable)
        cfgs = O.block_configs_quanonet(case.n, case.net)
    else:
        m = H.heaqnn(case.n, case.b_in, case.net, seed, scale_coeff=case.scale, if_trainable_freq=case.trainable)
        cfgs = O.block_configs_heaqnn(case.n, case.net)
    rng = np.random.default_rng(seed)
    branch = rng.normal(size=(case.batch, case.b_in))
    trunk = rng.uniform(size=(case.batch, case.t_in)) if case.kind == 'QuanONet' else None
    y = rng.normal(scale=0.5, size=case.batch)
    if case.reach is not None:
        sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
        enc = O.tiled_elementwise(branch, sd['branch_freq.weights'], sd['branch_freq.bias'])
        branch = branch * (case.reach / np.abs(enc).max())
    return m, cfgs, (branch, trunk, y)


def model_reference(case):
    """Reference of one model-level case: 'row' (the gradients in parameter order), 'sse' and 'out' (the predictions)"""
    key = ('model', case.id)
    if key not in _REFS:
        m, cfgs, (branch, trunk, y) = model_of(case)
        names = [k for k, _ in m.named_parameters()]
        sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
        kw = dict(ham_bound=HAM_BOUND, scale_coeff=case.scale)
        if case.kind == 'QuanONet':
            sse, grads, out = L.quanonet_loss_and_grads(sd, branch, trunk, y, case.n, case.net, **kw)
            f64 = [O.quanonet_loss_and_grads(sd, branch, trunk, y, case.n, case.net, engine=e, **kw) for e in (C, None)]
        else:
            sse, grads, out = L.heaqnn_loss_and_grads(sd, branch, y, case.n, case.net, **kw)
            f64 = [O.heaqnn_loss_and_grads(sd, branch, y, case.n, case.net, engine=e, **kw) for e in (C, None)]
        ld = {'row': tuple(np.concatenate([grads[k][i].reshape(-1) for k in names]) for i in (0, 1)),
              'sse': (np.array([sse[0]]), np.array([sse[1]])), 'out': out}
        errs = []
        for loss, g64, o64 in f64:
            row = np.concatenate([np.asarray(g64[k], np.float64).reshape(-1) for k in names])
            errs.append({'row': _maxabs(L.err(row, ld['row'])), 'sse': _maxabs(L.err([loss * len(y)], ld['sse'])),
                         'out': _maxabs(L.err(o64, ld['out']))})
        _REFS[key] = Reference((m, cfgs, branch, trunk, y), ld, errs[0], errs[1])
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------------------
# the code under test (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _t(dev, a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


def _named(launches, idents, want):
    """the one circuit kernel among the launches, asserted to be `want` = (identifier, template arguments); its name"""
    from tests.helpers import mangled_is
    hits = [(ident, name) for name, _, _ in launches for ident in idents if mangled_is(name, ident)]
    assert len(hits) == 1, [l[0] for l in launches]
    ident, name = hits[0]
    assert ident == want[0] and mangled_is(name, *want), (name, want)
    return name


def run_circuit_case(dev, case, cus):
    """The case on the device under its variant: ({quantity: float64 array}, {'fwd': kernel name, 'bwd': kernel name}).
    The kernels are asserted by name to be the case's, so that a budget is never credited to another kernel."""
    from quanonet_amd import _lib
    from tests.helpers import kernel_launches
    B = case.batch(cus)
    x, w, g, off, co, diag, pauli = circuit_reference(case, B).inputs
    sh = _lib.CircuitShape(case.n, case.cfgs)
    xd, wd, gd, dd = _t(dev, x), _t(dev, w), _t(dev, g), _t(dev, diag)
    _lib.set_backward_variant(case.variant)
    try:
        out, st = _lib.hea_forward(sh, xd, wd, off, co, dd, return_state=True, ham_pauli=pauli)
        gx, gw, out2 = _lib.hea_backward(sh, xd, wd, gd, off, co, dd, want_out=True, ham_pauli=pauli)
        _lib.check_status(dev)
        got = {'out': out.cpu().numpy(), 'state': st.cpu().numpy(), 'grad_x': gx.cpu().numpy(), 'grad_w': gw.cpu().numpy(),
               'backward out': out2.cpu().numpy()}
        fl = kernel_launches(dev, lambda: _lib.hea_forward(sh, xd, wd, off, co, dd, return_state=True, ham_pauli=pauli))
        bl = kernel_launches(dev, lambda: _lib.hea_backward(sh, xd, wd, gd, off, co, dd, want_out=True, ham_pauli=pauli))
    finally:
        _lib.set_backward_variant('auto')
        _lib.check_status(dev)
    return got, {'fwd': _named(fl, FWD_KERNELS, case.fwd), 'bwd': _named(bl, BWD_KERNELS, case.bwd)}


def run_model_case(dev, case, cus):
    """qhea_model_loss_grad, one call with the reference's parameters: ({'row', 'sse', 'out'}, {'bwd'}); the kernel
    asserted to be AUTO's at this batch (tests/test_dispatch_regimes.py: expected)"""
    import torch
    from quanonet_amd import _lib
    from tests.helpers import flat, kernel_launches
    m, cfgs, branch, trunk, y = model_reference(case).inputs
    want = expected(case.n, cfgs, case.batch, cus)
    desc = m.fused_desc()
    params = flat(m).to(dev).contiguous()
    P = params.numel()
    bd, td, yd = _t(dev, branch), _t(dev, trunk), _t(dev, y)
    grad = torch.zeros(P + 2, dtype=torch.float64, device=dev)
    pred = torch.zeros(case.batch, dtype=torch.float64, device=dev)

    def call():
        _lib.model_loss_grad(desc, bd, td, yd, params, 1.0 / case.batch, grad, pred=pred)
    call()
    _lib.check_status(dev)
    row = grad.cpu().numpy()
    got = {'row': row[:P].copy(), 'sse': row[P:P + 1].copy(), 'out': pred.cpu().numpy()}
    launches = kernel_launches(dev, call)
    _lib.check_status(dev)
    dense = (case.n, 2) if want.dense else None
    two = (case.n, want.pipes) if want.bwd == 'bwd_ztri_kernel' else dense
    return got, {'bwd': _named(launches, BWD_KERNELS, (want.bwd, two))}       # (the backward kernel does the forward sweep too)


def measure(got, ref, q, ld_q=None):
    """(max abs error of got[q] against the long-double value, e_ref, budget) of one quantity"""
    k = ld_q or q
    return _maxabs(L.err(got[q], ref.ld[k])), e_ref(ref, k), budget(ref, k)
