"""
Error budgets of the exact noisy forward kernels -- density_fwd_kernel<N> (hea_density.hip) and density_dev_fwd_kernel<N>
(hea_density_device.hip) for N = 2..6, and the tiled chain of hea_density_wide.hip for N = 7, 8, 9 -- the kernels every other noisy
number of the project is judged against.  Test infrastructure; importing it needs no GPU.  tests/test_forward_precision_oracle.py
(CPU) checks the references and the inputs, tests/test_forward_precision_budget.py (GPU) the kernels,
scripts/forward_precision_budget.py records the figures.

The rule is that of tests/precision_cases.py (FACTOR, ULP, Reference, e_ref, measure and _maxabs are imported from there, split and
_is from tests/density_precision_cases.py; nothing is restated):

    budget(q) = FACTOR * max( e_ref(q) , 2^-53 * scale(q) )

Quantities, from one forward call: 'pred' (pred[rows]) and 'sd' (shot_std[rows]).

q_ld is the channel-form reference in np.clongdouble on the same float64 inputs: density_reference.exact_moments (uniform family
and the wide chain) or device_noise_reference.device_moments (device family), with the model around the circuit -- frequency
layer or fixed scale, bias -- in the wide type too (density_grad_reference.model_circuit).  e_ref(q) is the larger error against
q_ld of two fp64 evaluations that differ from each other in the evolution and in the read-out:
  * Reference.e_c: the same function as q_ld in complex128 -- the confusion on the probabilities, the sums as matrix products;
  * Reference.e_np: a second form of the evolution -- uniform family: device_noise_reference.final_rho (Pauli mixtures, Kraus
    sums) under a uniform setting, equal p1 and p2 on every wire and slot, zero durations, idle off; device family: the stored
    walk's forward sweep, device_noise_grad_reference.stored_final_rho (one superoperator contraction per channel) -- read out the
    way the kernels do it (kernel_readout below): the confusion as n two-point mixes of the value tables h and h^2, then the 2^n
    products p_k h'_k added one after the other in index order.  numpy's pairwise product is more accurate than any sequential or
    lane-wise sum; with it in both evaluations e_ref would undercut a correct kernel.  This plays the part the inverse walk
    plays in the gradient tables.
No number of the code under test enters a budget.

scale(q).  Both quantities are cancelling sums: the read-outs are symmetric (HAM_BOUND, a diag table of mean zero), so pred comes
out at 1e-3 .. 0.2 from terms of magnitude up to 5 and 2^-53 max|pred| would say nothing about a sum's rounding.  The floor's
magnitude is therefore taken, in long double from q_ld's own p, h' and m1, m2, as
    scale(pred) = max_b sum_k p_k |h'_k|
    scale(sd)   = max_b (m2 / 2 + |m1| sum_k p_k |h'_k|) / sd         what one ulp on m2 and one on m1 move sqrt(m2 - m1^2) by.
It travels in Reference.ld as the entry 'scale:<q>', and budget() below hands that entry to precision_cases.budget: the rule has
one text.

Models.  Fixed-frequency HEAQNNs (blocks, LD) with one input column per encoding angle, inputs uniform in (-1, 1) and scale pi,
ansatz angles redrawn uniformly in (-pi, pi); read-out Z / X / Y scaled to [-5, 5], or for 'diag' a normal table of mean zero.
One trainable-frequency QuanONet per family (a HEAQNN has no bias; the QuanONets' is 0.1 x (seed + 1), never zero).  The
encoding-only HEAQNNs (2, 0) have a trainable frequency layer at its initial weights pi and biases 0 -- the same angles: with a
fixed scale such a model has no parameter at all, and the calls refuse a null parameter pointer.

Rows.  n <= 6: one more than the row slots of a workgroup of launch_density_fwd (row_slots reads them from the launcher's text):
a full workgroup and a second one with tail slots; every row is compared.  Wide chain: two rows at n = 7, 8 (row 1 shows
rho + (r << 2N) and csr), one at n = 9.

Noise.  Uniform family and wide chain: NOISES -- none, the README's rates, the rates the other tests use.  Device family:
tests/golden/device_calibration_5q.json at n = 5; elsewhere perwire_setting -- every wire its own p1, T1, T2, readout01 and
readout10, every ring slot its own p2, so that a swapped wire or slot index shows.

Lowered.  The condition on the inputs (tests/test_forward_precision_oracle.py) is budget(q) <= CAP for both quantities.  LOWERED
lists the planned cases whose references alone cannot meet it, with the figures, and the depth they run at instead.  Both are
noisy circuits at the README's depth, and in both it is sd that misses: a channel's coefficients are rounded once, so each
application moves Tr rho by a relative 1e-16 or so in one direction, m2 = sum p h'^2 follows the trace with a weight of 25 / 2 sd,
and e_ref(sd) grows in proportion to the number of sub-layers -- in any fp64 evaluation, the kernels' included.  The noiseless
case keeps the README's depth.
"""
import functools
import json
import os
import re
from collections import namedtuple

import numpy as np

from oracle import hea_oracle as O
from oracle.ld_oracle import err
from tests import density_grad_reference as DG
from tests import density_reference as DR
from tests import device_noise_grad_reference as DV
from tests import device_noise_reference as DNR
from tests import precision_cases as PC
from tests.density_precision_cases import split, _is
from tests.precision_cases import FACTOR, ULP, Reference, e_ref, measure as _measure, _maxabs        # noqa: F401 (the rule)

assert np.finfo(np.longdouble).nmant >= 63, 'np.longdouble is not wider than float64 here: no reference for these budgets'

WIDE = np.clongdouble
HAM_BOUND = (-5.0, 5.0)
SEED0 = 3800
CAP = 1e-12                                   # two orders below the atol the functional tests hold these kernels to
QUANTITIES = ('pred', 'sd')
NOISES = {'none': (0.0, 0.0, 0.0), 'readme': (1e-3, 1e-2, 0.01), 'heavy': (0.03, 0.08, 0.04)}       # (p1, p2, readout)
KERNEL = {'uniform': 'density_fwd_kernel', 'device': 'density_dev_fwd_kernel'}
WIDE_KERNELS = ('density_wide_ring_kernel', 'density_wide_wires_kernel', 'density_wide_readout_kernel')
# id of the planned case -> (its planned net, the net used, why).  Measured with the references alone (32 x e_ref(sd), to be at most
# CAP): see tests/test_forward_precision_oracle.py, which prints them.
# id -> the id of the case whose circuit, row and noise it shares; only the read-out basis differs, so the evolution -- 9 s of
# numpy at n = 9, most of it the Kraus form -- is computed once for the pair
SHARED = {'wide-q9-3x2-readme-X': 'wide-q9-3x2-readme', 'wide-q9-3x2-heavy-Y': 'wide-q9-3x2-heavy'}
LOWERED = {
    'uniform-q5-60x2-readme': ((60, 2), (20, 2), 'at (60, 2) the references give budget(sd) = 2.3e-12 (e_ref 7.3e-14, the fp64 channel '
                                                 'form); (40, 2) 1.7e-12, (30, 2) 1.2e-12, (25, 2) 9.6e-13; (20, 2) 8.0e-13'),
    'device-q5-60x2-calibration': ((60, 2), (8, 2), 'at (60, 2) the references give budget(sd) = 5.4e-12 (e_ref 1.7e-13, the fp64 stored '
                                                    'forward); (30, 2) 2.6e-12, (15, 2) 1.4e-12, (10, 2) 9.8e-13; (8, 2) 7.9e-13'),
}

Case = namedtuple('Case', 'id family n kind net readout noise rows')
# family: 'uniform' | 'device' (the kernel: KERNEL[family], template argument n) | 'wide' (WIDE_KERNELS at n).  kind / net: 'heaqnn'
# (blocks, LD) or 'quanonet' (branch depth, LD, trunk depth, LD).  noise: a key of NOISES, or 'calibration', 'perwire',
# 'perwire-noidle' (device family).


@functools.lru_cache(maxsize=None)
def row_slots(n):
    """the row slots of a workgroup of launch_density_fwd (hea_density.hpp), evaluated from the launcher's own expression"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'quanonet_amd', 'csrc', 'hea_density.hpp')
    with open(path) as f:
        src = f.read()
    threads = int(re.search(r'constexpr int kDensThreads = (\d+);', src).group(1))
    body = src[src.index('int launch_density_fwd('):]
    expr = re.search(r'constexpr int RPW = ([^;]+);', body).group(1)
    assert re.fullmatch(r'[\w\s()<>*/+-]+', expr), expr
    return int(eval(expr.replace('/', '//'), {'__builtins__': {}}, {'kDensThreads': threads, 'N': n}))


def _cases():
    out = []

    def name(family, n, net, readout, noise, kind):
        blocks = net[0] if kind == 'heaqnn' else net[0] + net[2]
        return f'{family}-q{n}-{blocks}x{net[1]}-{noise}' + ('' if readout == 'Z' else f'-{readout}') + \
            ('-trainable' if kind == 'quanonet' else '')

    def add(family, n, net, readout, noise, kind='heaqnn'):
        cid = name(family, n, net, readout, noise, kind)
        if cid in LOWERED:
            assert LOWERED[cid][0] == net
            net = LOWERED[cid][1]
            cid = name(family, n, net, readout, noise, kind)
        rows = (1 if n == 9 else 2) if family == 'wide' else row_slots(n) + 1
        out.append(Case(cid, family, n, kind, net, readout, noise, rows))

    small = {2: 'Z', 3: 'X', 4: 'Y', 5: 'diag', 6: 'Z'}
    # density_fwd_kernel<N>
    for n in (2, 3, 4, 5, 6):
        for noise in NOISES:
            add('uniform', n, (3, 2), small[n], noise)
    for noise in ('none', 'readme'):
        add('uniform', 5, (60, 2), 'Z', noise)                           # the depths that are trained
    add('uniform', 6, (10, 2), 'Z', 'readme')
    for n, readout in ((3, 'Y'), (4, 'Z')):                              # (RX on |0> has no X component: <X> = 0 in every row)
        add('uniform', n, (2, 0), readout, 'heavy')                      # encoding blocks only: wire_passes, odd and even n
    add('uniform', 4, (2, 2, 1, 2), 'Z', 'readme', kind='quanonet')
    # density_dev_fwd_kernel<N>
    add('device', 5, (3, 2), 'Z', 'calibration')
    add('device', 5, (3, 2), 'diag', 'calibration')
    add('device', 5, (60, 2), 'Z', 'calibration')
    for n in (2, 3, 4, 6):
        add('device', n, (3, 2), small[n], 'perwire')
    add('device', 4, (3, 2), 'Z', 'perwire-noidle')
    add('device', 3, (2, 0), 'Z', 'perwire')                             # dev_enc_passes
    add('device', 3, (2, 2, 1, 2), 'Z', 'perwire', kind='quanonet')
    # the wide chain
    for n, readout in ((7, 'Z'), (8, 'diag'), (9, 'Z')):
        for noise in NOISES:
            add('wide', n, (3, 2), readout, noise)
    add('wide', 8, (2, 0), 'Z', 'heavy')                                 # stage B serves exactly one pair: wide_wire_pass<8, 1, 4>
    add('wide', 8, (2, 0, 1, 2), 'X', 'readme', kind='quanonet')         # ... behind a sub-layer stage, and in the basis change
    add('wide', 9, (3, 2), 'X', 'readme')
    add('wide', 9, (3, 2), 'Y', 'heavy')
    return out


CASES = _cases()


def cfgs_of(case):
    return (O.block_configs_quanonet if case.kind == 'quanonet' else O.block_configs_heaqnn)(case.n, case.net)


def perwire_setting(n, idle=True):
    """a device setting in which no two wires and no two ring slots agree (in the range of the golden calibration, times in us)"""
    from quanonet_amd.noise import DeviceNoise
    q = np.arange(n)
    return DeviceNoise(p1=tuple(1e-3 * (1 + q)), p2=tuple(5e-3 * (2 + (3 * q) % n) + 1e-3 * q), readout01=tuple(0.01 + 0.004 * q),
                       readout10=tuple(0.03 + 0.005 * ((q + 2) % n) + 0.0013 * q), t1=tuple(80.0 + 17.0 * q),
                       t2=tuple(60.0 + 23.0 * ((q + 1) % n) + 2.0 * q), t_rx=0.07, t_rot=0.07, t_cx=0.4, idle=idle)


def calibration_setting():
    from quanonet_amd.noise import DeviceNoise
    from tests.helpers import GOLDEN
    with open(os.path.join(GOLDEN, 'device_calibration_5q.json')) as f:
        return DeviceNoise.from_calibration(json.load(f), [0, 1, 2, 3, 4])


_INPUTS = {}
Inputs = namedtuple('Inputs', 'model spec flat branch trunk noise')
# model: the fp64 torch model on the CPU.  noise: quanonet_amd.noise.NoiseModel (uniform, wide) or DeviceNoise.


def inputs_of(case):
    """the case's model, rows and noise setting, made once"""
    if case.id in _INPUTS:
        return _INPUTS[case.id]
    import torch
    from quanonet_amd.noise import NoiseModel
    from tests import helpers as H
    n = case.n
    seed = SEED0 + [c.id for c in CASES].index(SHARED.get(case.id, case.id))
    rng = np.random.default_rng(seed)
    kw = dict(scale_coeff=np.pi, ham_bound=HAM_BOUND)
    if case.readout == 'diag':
        diag = rng.normal(size=1 << n)
        kw['ham_diag'] = diag - diag.mean()
    else:
        kw['ham_pauli'] = case.readout
    if case.kind == 'quanonet':
        m = H.quanonet(n, 6, 2, case.net, seed - SEED0, if_trainable_freq=True, **kw)       # (the model's bias is 0.1 x (its seed + 1))
        branch, trunk = rng.uniform(-1, 1, (case.rows, 6)), rng.uniform(-1, 1, (case.rows, 2))
    else:
        m = H.heaqnn(n, n * case.net[0], case.net, seed - SEED0, if_trainable_freq=case.net[1] == 0, **kw)
        branch, trunk = rng.uniform(-1, 1, (case.rows, n * case.net[0])), None
    with torch.no_grad():
        w = m.quantum_layer.ansatz_weights
        w.copy_(torch.from_numpy(rng.uniform(-np.pi, np.pi, tuple(w.shape))))
    if case.noise in NOISES:
        p1, p2, readout = NOISES[case.noise]
        noise = NoiseModel(p1=p1, p2=p2, readout=readout)
    else:
        noise = calibration_setting() if case.noise == 'calibration' else perwire_setting(n, idle=case.noise == 'perwire')
    _INPUTS[case.id] = Inputs(m, DG.spec_of(m), H.flat(m).numpy(), branch, trunk, noise)
    return _INPUTS[case.id]


def noise_dict(case):
    """the case's noise as the dict device_noise_reference takes; a uniform setting as equal rates on every wire and slot,
    zero durations, idle off"""
    from tests.test_device_noise_training_abi import as_dict
    nz, n = inputs_of(case).noise, case.n
    if case.noise not in NOISES:
        return as_dict(nz, n)
    return dict(p1=[nz.p1] * n, p2=[nz.p2] * n, readout01=[nz.readout] * n, readout10=[nz.readout] * n, t1=[np.inf] * n,
                t2=[np.inf] * n, t_rx=0.0, t_rot=0.0, t_cx=0.0, idle=False)


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def kernel_readout(prob, n, readout01, readout10, hv):
    """
    (m1[B], m2[B]) from outcome probabilities prob[B, 2^n] the way the kernels do it, in fp64: the confusion applied to the
    value tables -- per bit i, h'[k] = (1 - f) h[k] + f h[k ^ 1 << i] with f = P(bit i of k is misread), for h and h^2 -- and the
    2^n products added one after the other in index order.
    """
    D = 1 << n
    kk = np.arange(D)
    h = np.array(hv, np.float64)
    h2 = h * h
    for i in range(n):
        f = np.where((kk >> i) & 1, np.float64(readout10[i]), np.float64(readout01[i]))
        h, h2 = (1.0 - f) * h + f * h[kk ^ (1 << i)], (1.0 - f) * h2 + f * h2[kk ^ (1 << i)]
    prob = np.asarray(prob, np.float64)
    m1, m2 = np.zeros(prob.shape[0]), np.zeros(prob.shape[0])
    for k in range(D):
        m1 += prob[:, k] * h[k]
        m2 += prob[:, k] * h2[k]
    return m1, m2


_PROBS = {}


def probabilities(case, form, dtype=np.complex128):
    """(diag rho [rows, 2^n] in the real type of dtype, the bias) of the case, computed once per process.  form: 'channel' (the
    closed channel forms of density_reference; for the device family the Kraus timeline of device_noise_reference, what q_ld is
    made of) or 'second' (the other arithmetic: see the head of this file)"""
    key = (case.id, form, np.dtype(dtype))
    if key not in _PROBS:
        _PROBS[key] = _probabilities(case, form, dtype)
        _PROBS[key][0].setflags(write=False)
    return _PROBS[key]


_EVOLVED = {}


def _probabilities(case, form, dtype):
    i = inputs_of(case)
    mc = DG.model_circuit(i.spec, i.flat, i.branch, i.trunk, dtype)
    n, D = mc.n, 1 << mc.n
    key = (SHARED.get(case.id, case.id), form, np.dtype(dtype))
    if key in _EVOLVED:
        rho = _EVOLVED[key]
    else:                                                                # rho before the basis change of the read-out
        if case.family == 'device':
            rho_of = DNR.final_rho if form == 'channel' else DV.stored_final_rho
            rho = rho_of(n, mc.cfgs, mc.x, mc.w, noise_dict(case), 'Z', dtype)
        elif form == 'channel':
            rho = DR.final_rho(n, mc.cfgs, mc.x, mc.w, i.noise.p1, i.noise.p2, 'Z', dtype)
        else:
            rho = DNR.final_rho(n, mc.cfgs, mc.x, mc.w, noise_dict(case), 'Z', dtype)
        if key[0] in SHARED.values():
            _EVOLVED[key] = rho
    literal = form == ('channel' if case.family == 'device' else 'second')      # rho is device_noise_reference.final_rho's
    change = DNR.basis_change if literal else DR.basis_change                   # each form keeps its own basis change
    rho = np.ascontiguousarray(change(rho.reshape((-1,) + (2,) * (2 * n)), n, i.spec['ham_pauli'])).reshape(-1, D, D)
    return np.real(np.einsum('bkk->bk', rho)), (mc.flat[0] if mc.quanonet else DR.real_of(dtype)(0.0))


def pairwise_moments(case, prob):
    """(mean, var) without the bias by the read-out of the case's channel-form reference, in prob's type"""
    s = inputs_of(case).spec
    if case.family == 'device':
        return DNR.moments_of(prob, case.n, noise_dict(case), s['offset'], s['coeff'], s['ham_diag'])
    return DR.moments_of(prob, case.n, inputs_of(case).noise.readout, s['offset'], s['coeff'], s['ham_diag'])


def _sd(var):
    return np.sqrt(np.maximum(var, 0))


def evaluate(case, form, dtype=np.complex128):
    """{'pred', 'sd'} of the case by one of the two forms; the second form exists in fp64 only"""
    prob, bias = probabilities(case, form, dtype)
    if form == 'channel':
        mean, var = pairwise_moments(case, prob)
    else:
        assert np.dtype(dtype) == np.complex128
        s, nz = inputs_of(case).spec, noise_dict(case)
        m1, m2 = kernel_readout(prob, case.n, nz['readout01'], nz['readout10'],
                                DNR.value_table(case.n, s['offset'], s['coeff'], s['ham_diag']))
        mean, var = m1, m2 - m1 * m1
    return {'pred': mean + bias, 'sd': _sd(var)}


def scales(case, prob):
    """{'pred', 'sd'}: the magnitudes the floor of the budget refers to (the head of this file), in prob's wide type"""
    i = inputs_of(case)
    s = i.spec
    if case.family == 'device':
        hv = DV.value_table(case.n, noise_dict(case), s['offset'], s['coeff'], s['ham_diag'], WIDE)
    else:
        hv = DG.value_table(case.n, i.noise.readout, s['offset'], s['coeff'], s['ham_diag'], WIDE)
    m1, var = pairwise_moments(case, prob)
    mass = prob @ np.abs(hv)
    return {'pred': mass.max(), 'sd': (((var + m1 * m1) / 2 + np.abs(m1) * mass) / _sd(var)).max()}


_REFS = {}


def reference(case):
    """Reference (tests/precision_cases.py) of one case, computed once per process: ld = q_ld as (hi, lo) pairs with the
    entries 'scale:pred' and 'scale:sd' beside them, e_c = the fp64 channel form's error against q_ld, e_np = the second form's"""
    if case.id not in _REFS:
        prob, bias = probabilities(case, 'channel', WIDE)
        mean, var = pairwise_moments(case, prob)
        ld = {'pred': split(mean + bias), 'sd': split(_sd(var))}
        for q, v in scales(case, prob).items():
            ld['scale:' + q] = split(v)
        errs = [{q: _maxabs(err(v, ld[q])) for q, v in evaluate(case, form).items()} for form in ('channel', 'second')]
        for pair in ld.values():
            for a in pair:
                a.setflags(write=False)
        _REFS[case.id] = Reference(inputs_of(case), ld, errs[0], errs[1])
    return _REFS[case.id]


def scale(ref, q):
    return _maxabs(ref.ld['scale:' + q][0])


def budget(ref, q):
    """precision_cases.budget with scale(q) in the place of max|q_ld|"""
    return PC.budget(ref._replace(ld={q: ref.ld['scale:' + q]}), q)


def measure(got, ref, q):
    """(max abs error of got[q] against q_ld, e_ref, budget) of one quantity"""
    error, e, _ = _measure(got, ref, q)
    return error, e, budget(ref, q)


# ---------------------------------------------------------------------------------------------------------------------
# the code under test (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def run_case(dev, case):
    """The case's one forward call on the device: ({'pred', 'sd'}, the mangled names of the family's kernels that ran).  They
    are asserted by name and first template argument to be the case's, so that a budget is never credited to another kernel:
    n <= 6 exactly one density_fwd_kernel<n> or density_dev_fwd_kernel<n> on two workgroups; the wide chain the stage kernels
    its circuit needs and the read-out kernel, all at n, and neither of the n <= 6 kernels."""
    import torch
    from quanonet_amd import _lib
    from tests.helpers import kernel_launches, mangled_is
    i = inputs_of(case)
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    desc = i.model.fused_desc()
    flat, branch, trunk = t(i.flat), t(i.branch), t(i.trunk)
    q = i.model.quantum_layer
    diag = q.ham_diag.to(dev) if q.use_full_ham else None
    pred = torch.full((case.rows,), float('nan'), dtype=torch.float64, device=dev)
    sd = torch.full((case.rows,), float('nan'), dtype=torch.float64, device=dev)
    entry, rec = {'uniform': (_lib.model_forward_noisy_exact, None), 'wide': (_lib.model_forward_noisy_exact_wide, None),
                  'device': (_lib.model_forward_noisy_device_exact, case.n)}[case.family]
    rec = i.noise.params() if rec is None else i.noise.params(rec)

    def call():
        entry(desc, branch, trunk, flat, rec, ham_diag=diag, out=pred, shot_std=sd)
    call()
    _lib.check_status(dev)
    torch.cuda.synchronize()
    got = {'pred': pred.cpu().numpy(), 'sd': sd.cpu().numpy()}
    launches = kernel_launches(dev, call)
    _lib.check_status(dev)
    small = [k for k in launches for ident in KERNEL.values() if _is(mangled_is, k[0], ident)]
    names = [k[0] for k in launches]
    if case.family != 'wide':
        assert len(small) == 1, names
        name, grid, _ = small[0]
        assert _is(mangled_is, name, KERNEL[case.family], (case.n,)), (name, KERNEL[case.family], case.n)
        assert grid == (2, 1, 1), (grid, case.rows)                      # a full workgroup and one with tail slots
        return got, [name]
    assert not small, names
    ring, wires, readout = ([k for k in names if _is(mangled_is, k, ident)] for ident in WIDE_KERNELS)
    cfgs = cfgs_of(case)
    assert bool(ring) == any(ld > 0 for _, ld in cfgs), names
    assert bool(wires) == (any(ld == 0 for _, ld in cfgs) or case.readout in ('X', 'Y')), names
    assert len(readout) == 1, names
    for k, ident in [(k, WIDE_KERNELS[0]) for k in ring] + [(k, WIDE_KERNELS[1]) for k in wires] + [(readout[0], WIDE_KERNELS[2])]:
        assert _is(mangled_is, k, ident, (case.n,)), (k, ident, case.n)
    return got, sorted(set(ring + wires + readout))
