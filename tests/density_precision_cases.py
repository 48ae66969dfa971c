"""
Error budgets of the three density-matrix gradient kernels -- density_bwd_kernel<N> (hea_density_grad.hip),
density_dev_bwd_kernel<N> and density_dev_stored_bwd_kernel<N> (hea_density_device_grad.hip) -- from log10 A = 0 to their guards,
at the depths that are trained.  Test infrastructure; importing it needs no GPU.  tests/test_density_precision_oracle.py (CPU)
checks the references and the inputs, tests/test_density_precision_budget.py (GPU) the kernels,
scripts/density_precision_budget.py records the figures.

The rule is that of tests/precision_cases.py (FACTOR, ULP, e_ref, budget and measure are imported from there, not restated):

    budget(q) = FACTOR * max( e_ref(q) , 2^-53 * max|q_ld| )

with q_ld the helper's stored walk evaluated in np.clongdouble on the same float64 inputs (density_grad_reference /
device_noise_grad_reference, dtype=np.clongdouble: angles, sin / cos / exp, channel coefficients, the model around the circuit
and every sum in the wide type) and e_ref(q) the larger error against q_ld of the two fp64 numpy evaluations: the helper's
stored walk (inverse=False; Reference.e_c) and its inverse walk (inverse=True; Reference.e_np), which has the conditioning the
kernels have.  For a stored-kernel case past the inverse walk's guard only the fp64 stored walk enters (e_np = 0): marked
`past` below.  No number of the code under test enters a budget.

Quantities, from one loss_grad call: 'row' (grad[:P]), 'sse' (grad[P]) and 'pred'.

Models.  Fixed-frequency HEAQNNs (blocks, LD) with one input column per encoding angle, inputs uniform in (-1, 1) and scale pi,
ansatz angles redrawn uniformly in (-pi, pi): every angle of the circuit covers the circle.  One trainable-frequency QuanONet
Q5 Net20-2-10-2 (30 blocks of LD 2) on 3 rows puts the frequency weights' entries, sums over rows of grad_x * in, under a budget.
The past-the-guard stored case is tests/test_device_noise_stored_training.py's past_the_bound_case as it is.

Rows.  n >= 5: one row (a workgroup holds one row).  n <= 4: a workgroup of launch_density_bwd holds 64 / 4^(n-2) = 64, 16, 4 row
slots; ROWS_SMALL = 2 is the smallest count that fills more than one slot and leaves a tail slot at each of them.

Noise.  Uniform family: p2 = 6 p1 with log10 A = target (test_noise_aware_abi._rates_for), readout 0.01; one case runs the
README's rates as they are (p1 = 1e-3, p2 = 1e-2 on 120 sub-layers: 3.3).  Device family: test_device_noise_training_abi's
probe_setting(n, cfgs, target, idle=True) -- relaxation on every wire but one, idle decay on.

Lowered target.  The condition on the inputs (tests/test_density_precision_oracle.py) is budget(row) <= 2^-10 max|row_ld|.
LOWERED lists the cases whose references alone cannot meet it at the planned target, with the figures.
"""
from collections import namedtuple

import numpy as np

from oracle import hea_oracle as O
from oracle.ld_oracle import err
from tests import density_grad_reference as DG
from tests import device_noise_grad_reference as DV
from tests.precision_cases import FACTOR, ULP, Reference, budget, e_ref, measure, _maxabs        # noqa: F401 (the rule)

assert np.finfo(np.longdouble).nmant >= 63, 'np.longdouble is not wider than float64 here: no reference for these budgets'

WIDE = np.clongdouble
READOUT = 0.01                                # the uniform family's readout flip probability
README_RATES = (1e-3, 1e-2)                   # README / DESIGN 7f: Q5 Net40-2-20-2 at these rates has log10 A = 3.3
ROWS_SMALL = 2
SEED0 = 3500
HAM_BOUND = (-5.0, 5.0)                       # the models' default: read values n - 2 popcount scaled to [-5, 5], no offset
# The identity component of the read-out.  Im Tr(O sigma rho) does not see a multiple of the identity in O, so a read-out
# offset changes pred and no derivative of pred; a kernel that leaves it in O multiplies it with the rounding residue of the
# inverse walk on rho, which grows with A (measured before density_bwd_kernel removed it: error 8e-7 on gradients of 6e-11 at
# log10 A = 11.99 with an offset of 0.5; the fp64 numpy inverse walk does the same, 8e-7).  The table's read-outs therefore have
# none (HAM_BOUND is symmetric, the diag case's table has mean zero), and the '-offset' cases add IDENTITY to the read-out of a
# twin case and to its targets y: same circuit, same residuals pred - y, mathematically the same row.  Their e_ref takes the
# fp64 stored walk on their own inputs and the fp64 inverse walk of the twin -- what the inverse walk costs on this circuit
# without the component that carries no gradient; their q_ld is the wide stored walk on their own inputs.  Uniform family only:
# under device noise relaxation makes identity out of Z at every site (b != 0), which is what its lower guard answers.
IDENTITY = 0.5
GUARD = {'uniform': 12.0, 'device': 7.0, 'stored': 7.0}      # the constants of the library: total, total, per unit
KERNEL = {'uniform': 'density_bwd_kernel', 'device': 'density_dev_bwd_kernel', 'stored': 'density_dev_stored_bwd_kernel'}
QUANTITIES = ('row', 'sse', 'pred')

Case = namedtuple('Case', 'id family n kind net target rates readout rows past twin')
# family: 'uniform' | 'device' | 'stored' (the kernel: KERNEL[family], template argument n).  kind / net: 'heaqnn' (blocks, LD) or
# 'quanonet' (branch depth, LD, trunk depth, LD).  target: log10 A (uniform) or log10 A_dev.  rates: None, or the uniform
# family's (p1, p2) given as they are.  past: beyond the inverse walk's guard (stored family only).  twin: None, or the id of the
# case whose circuit, rows and noise this one shares, with IDENTITY added to its read-out and to its targets (see IDENTITY).

# id of the planned case -> (its planned target, the target used, why).  Measured with the references alone (32 x e_ref(row) /
# max|row_ld|, to be at most 2^-10 = 9.8e-4): see tests/test_density_precision_oracle.py, which prints them.
LOWERED = {'uniform-q2-30x2-A11.99': (11.99, 10.0, 'at 11.99 the references give 32 x e_ref(row) / max|row| = 1.6e-3 (e_ref 7.1e-16, the '
                                                      'fp64 inverse walk, on a largest entry of 1.4e-11): above 2^-10; at 10 it is 2.6e-5')}


def _uniform_target(n, cfgs, rates):
    return float(DG.log10_amplification(n, cfgs, *rates))


def _cases():
    out = []

    def add(family, n, net, target, readout='Z', kind='heaqnn', rates=None, past=False):
        blocks = net[0] if kind == 'heaqnn' else net[0] + net[2]
        name = f'{family}-q{n}-{blocks}x{net[1]}'
        if name + f'-A{target:g}' in LOWERED:
            target = LOWERED[name + f'-A{target:g}'][1]
        tag = 'readme' if rates else f'A{target:g}'
        cid = f'{name}-{tag}' + ('' if readout == 'Z' else f'-{readout}') + ('-trainable' if kind == 'quanonet' else '')
        rows = 3 if kind == 'quanonet' else 1 if n >= 5 else ROWS_SMALL
        out.append(Case(cid, family, n, kind, net, target, rates, readout, rows, past, None))
        return out[-1]

    small = {2: 'Z', 3: 'X', 4: 'Y'}
    # density_bwd_kernel<N>
    for target in (0.0, 4.0, 8.0, 11.99):
        add('uniform', 5, (30, 2), target, readout='diag' if target == 8.0 else 'Z')
    add('uniform', 5, (60, 2), _uniform_target(5, [(5, 2)] * 60, README_RATES), rates=README_RATES)
    add('uniform', 5, (60, 2), 11.99)
    for target in (0.0, 8.0, 11.99):
        add('uniform', 6, (10, 2), target)
    for n in (2, 3, 4):
        for target in (8.0, 11.99):
            add('uniform', n, (30, 2), target, readout=small[n])
    add('uniform', 5, (20, 2, 10, 2), 8.0, kind='quanonet')
    for twin in ('uniform-q5-30x2-A11.99', 'uniform-q5-30x2-A8-diag', 'uniform-q3-30x2-A11.99-X'):
        out.append(next(c for c in out if c.id == twin)._replace(id=twin + '-offset', twin=twin))
    # density_dev_bwd_kernel<N>
    for n, net in ((5, (30, 2)), (6, (10, 2))):
        for target in (0.0, 4.0, 7.0):
            add('device', n, net, target)
    add('device', 5, (60, 2), 7.0)
    for n in (2, 3, 4):
        add('device', n, (30, 2), 7.0, readout=small[n])
    # density_dev_stored_bwd_kernel<N>
    add('stored', 5, (30, 2), 7.0)
    add('stored', 3, (30, 2), 7.0, readout='X')
    add('stored', 3, (6, 2), 16.0, past=True)                # past the inverse walk's guard: e_ref is the fp64 stored walk's alone
    return out


CASES = _cases()


def cfgs_of(case):
    return (O.block_configs_quanonet if case.kind == 'quanonet' else O.block_configs_heaqnn)(case.n, case.net)


# case id -> seed, where the default (the case's position in the table) breaks the condition on the inputs that
# tests/test_density_precision_oracle.py states: a target y_b that happens to lie within |pred_b| / 8 of pred_b.  The row is
# sum_b 2 (pred_b - y_b) / B * d pred_b; there the rounding of pred alone, 2^-53 |pred_b| in any fp64 evaluation, is a larger
# part of the row than the 2^-53 max|row| that the budget's floor allows for, and e_ref covers it only if both numpy walks
# happen to round pred the same way as each other and otherwise than the kernel.
SEEDS = {'device-q6-10x2-A0': 101}


def _seed(case):
    key = case.twin or case.id
    return SEED0 + SEEDS.get(key, [c.id for c in CASES].index(key))


_INPUTS = {}
Inputs = namedtuple('Inputs', 'model spec flat branch trunk y noise logA')
# model: the fp64 torch model on the CPU.  noise: quanonet_amd.noise.NoiseModel (uniform) or DeviceNoise.  logA: the helper's
# log10 A / A_dev of the case's circuit under it.


def inputs_of(case):
    """the case's model, rows and noise setting, made once"""
    if case.id in _INPUTS:
        return _INPUTS[case.id]
    import torch
    from quanonet_amd.noise import NoiseModel
    from tests import helpers as H
    from tests.test_device_noise_training_abi import probe_setting
    from tests.test_noise_aware_abi import _rates_for
    n, cfgs, seed = case.n, cfgs_of(case), _seed(case)
    rng = np.random.default_rng(seed)
    if case.past:
        from tests.test_device_noise_stored_training import past_the_bound_case, past_the_bound_model
        assert case.readout == 'Z'
        spec, flat, x, y, noise, logA = past_the_bound_case(n, case.net, case.target, case.rows)
        _INPUTS[case.id] = Inputs(past_the_bound_model(n, case.net), spec, flat, x, None, y, noise, logA)
        return _INPUTS[case.id]
    shift = IDENTITY if case.twin else 0.0
    kw = dict(scale_coeff=np.pi, ham_bound=(HAM_BOUND[0] + shift, HAM_BOUND[1] + shift))
    if case.readout == 'diag':
        diag = rng.normal(size=1 << n)
        kw['ham_diag'] = diag - diag.mean() + shift
    else:
        kw['ham_pauli'] = case.readout
    if case.kind == 'quanonet':
        m = H.quanonet(n, 6, 2, case.net, seed - SEED0, if_trainable_freq=True, **kw)       # (the model's bias is 0.1 x (its seed + 1))
        branch, trunk = rng.uniform(-1, 1, (case.rows, 6)), rng.uniform(-1, 1, (case.rows, 2))
    else:
        m = H.heaqnn(n, n * case.net[0], case.net, seed - SEED0, if_trainable_freq=False, **kw)
        branch, trunk = rng.uniform(-1, 1, (case.rows, n * case.net[0])), None
    with torch.no_grad():
        w = m.quantum_layer.ansatz_weights
        w.copy_(torch.from_numpy(rng.uniform(-np.pi, np.pi, tuple(w.shape))))
    y = rng.normal(scale=0.7, size=case.rows) + shift
    if case.family == 'uniform':
        E, blk = n * len(cfgs), sum(ld for _, ld in cfgs)
        p1, p2 = case.rates or _rates_for(n, E, blk, case.target)
        noise, logA = NoiseModel(p1=p1, p2=p2, readout=READOUT), float(DG.log10_amplification(n, cfgs, p1, p2))
    else:
        # a setting bisected to the guard itself lands on either side of it in the library's own sum: stay 5e-7 inside
        at_guard = case.target == GUARD['device']
        noise, logA = probe_setting(n, cfgs, case.target - (5e-7 if at_guard else 0.0), idle=True)
    _INPUTS[case.id] = Inputs(m, DG.spec_of(m), H.flat(m).numpy(), branch, trunk, y, noise, float(logA))
    return _INPUTS[case.id]


def walk(case, inverse=False, dtype=np.complex128):
    """([P + 2] buffer, pred[rows]) of the case by the numpy helper of its family"""
    i = inputs_of(case)
    inv = 1.0 / case.rows
    if case.family == 'uniform':
        return DG.model_loss_grad(i.spec, i.flat, i.branch, i.trunk, i.y, i.noise.p1, i.noise.p2, i.noise.readout, inv,
                                  inverse=inverse, dtype=dtype)
    from tests.test_device_noise_training_abi import as_dict
    return DV.model_loss_grad(i.spec, i.flat, i.branch, i.trunk, i.y, as_dict(i.noise, case.n), inv, inverse=inverse, dtype=dtype)


def split(ref):
    """a wide array as the (hi, lo) pair of float64 arrays oracle.ld_oracle.err takes"""
    ref = np.atleast_1d(ref)
    hi = ref.astype(np.float64)
    return hi, (ref - hi).astype(np.float64)


def quantities(buf, pred):
    P = buf.shape[0] - 2
    return {'row': buf[:P], 'sse': buf[P:P + 1], 'pred': pred}


_REFS = {}


def reference(case):
    """Reference (tests/precision_cases.py) of one case, computed once per process: ld = the wide stored walk as (hi, lo) pairs,
    e_c = the fp64 stored walk's error against it, e_np = the fp64 inverse walk's (zeros past its guard)"""
    if case.id not in _REFS:
        ld = {q: split(v) for q, v in quantities(*walk(case, dtype=WIDE)).items()}
        stored = quantities(*walk(case))
        e_stored = {q: _maxabs(err(stored[q], ld[q])) for q in QUANTITIES}
        if case.past:
            e_inverse = {q: 0.0 for q in QUANTITIES}
        elif case.twin:
            e_inverse = reference(next(c for c in CASES if c.id == case.twin)).e_np
        else:
            inverse = quantities(*walk(case, inverse=True))
            e_inverse = {q: _maxabs(err(inverse[q], ld[q])) for q in QUANTITIES}
        for pair in ld.values():
            for a in pair:
                a.setflags(write=False)
        _REFS[case.id] = Reference(inputs_of(case), ld, e_stored, e_inverse)
    return _REFS[case.id]


# ---------------------------------------------------------------------------------------------------------------------
# the code under test (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def run_case(dev, case):
    """The case's one loss_grad call on the device: ({'row', 'sse', 'pred'}, the kernel's mangled name).  The kernel is asserted
    by name to be the case's family's, instantiated for the case's n, so that a budget is never credited to another kernel."""
    import torch
    from quanonet_amd import _lib
    from tests.helpers import kernel_launches, mangled_is
    i = inputs_of(case)
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    desc = i.model.fused_desc()
    flat, branch, trunk, y = t(i.flat), t(i.branch), t(i.trunk), t(i.y)
    q = i.model.quantum_layer
    diag = q.ham_diag.to(dev) if q.use_full_ham else None
    grad = torch.full((flat.numel() + 2,), float('nan'), dtype=torch.float64, device=dev)
    pred = torch.full((case.rows,), float('nan'), dtype=torch.float64, device=dev)
    if case.family == 'uniform':
        entry, rec = _lib.model_loss_grad_noisy_exact, i.noise.params()
    else:
        entry = _lib.model_loss_grad_noisy_device_exact_stored if case.family == 'stored' else _lib.model_loss_grad_noisy_device_exact
        rec = i.noise.params(case.n)

    def call():
        entry(desc, branch, trunk, y, flat, rec, 1.0 / case.rows, grad, ham_diag=diag, pred=pred)
    call()
    _lib.check_status(dev)
    torch.cuda.synchronize()
    got = quantities(grad.cpu().numpy(), pred.cpu().numpy())
    launches = kernel_launches(dev, call)
    _lib.check_status(dev)
    hits = [name for name, _, _ in launches for ident in KERNEL.values() if _is(mangled_is, name, ident)]
    assert len(hits) == 1, [l[0] for l in launches]
    assert _is(mangled_is, hits[0], KERNEL[case.family], (case.n,)), (hits[0], KERNEL[case.family], case.n)
    return got, hits[0]


def _is(mangled_is, name, ident, targs=None):
    """helpers.mangled_is for a kernel of an unnamed namespace: there the length-prefixed identifier follows '_GLOBAL__N_1',
    whose last digit mangled_is would take for part of the length; put a separator between the two"""
    return mangled_is(name.replace('_GLOBAL__N_1', '_GLOBAL__N_1_'), ident, targs)
