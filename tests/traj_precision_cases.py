"""
Error budgets of the four trajectory gradient units that train under noise at n = 7..12 -- noisy_grad_wave_kernel<N>
(hea_noise_grad.hip), noisy_grad_lds_kernel<N> (hea_noise_grad_lds.hip), device_grad_wave_kernel<N> (hea_noise_device_grad.hip)
and device_grad_lds_kernel<N> (hea_noise_device_grad_lds.hip) -- at depths that are trained.  Test infrastructure; importing it
needs no GPU.  tests/test_traj_precision_oracle.py (CPU) checks the references and the inputs,
tests/test_traj_precision_budget.py (GPU) the kernels, scripts/traj_precision_budget.py records the figures.

The rule is that of tests/precision_cases.py (FACTOR, ULP, Reference, e_ref, budget and measure are imported, not restated):

    budget(q) = FACTOR * max( e_ref(q) , 2^-53 * max|q_ld| )

q_ld is the numpy walk in np.clongdouble on the same float64 inputs (dtype=WIDE: angles, sin / cos / exp, sqrt(1 - gamma), the
read-out weights, the model around the circuit and every sum; the random words and the thresholds stay integers).  e_ref(q) is
the larger error against q_ld of two fp64 numpy evaluations (Reference.e_c, Reference.e_np):
  * sampled family (Pauli insertions, unitary): the adjoint walk traj_grad and the two-term shift of traj_grad_shift, evaluated
    at SHIFTED_ANGLES of the angles (_shift_form says why that never widens a budget);
  * jump family: the stored walk and the inverse walk (device_traj_grad_reference.walk, inverse=True, with the library's restart
    rule restart_above=RESTART_ABOVE -- none), which has the conditioning the kernels have.
No number of the code under test enters a budget.  Quantities, from one loss_grad call: 'row' (grad[:P]), 'sse' (grad[P]), 'pred'.

Models.  Fixed-frequency HEAQNNs (blocks, LD) with one input column per encoding angle, inputs uniform in (-1, 1) and scale pi,
ansatz angles redrawn uniformly in (-pi, pi), read-out scaled to [-5, 5] (a normal table of mean zero for 'diag').  The n = 9
sampled case is a trainable-frequency QuanONet Net2-2-1-2 (3 blocks of LD 2).  T = 5 trajectories: a full tile of 4 and a tile
of one.  Two rows in the sampled family (one at n = 12), one row in the jump family.

Jump settings.  t1 uniform in (0.8, 1.4) per wire, t2 = t1, the three durations equal to `tau`, Pauli rates 1e-3 / 1e-2, an
asymmetric read-out.  The realistic level has idle decay on and tau = 0.004 (gamma 3e-3 .. 0.05 over the sites); the others have
it off, so that every site of a wire has the same gamma = 1 - exp(-tau / t1).  A jump on any wire restores psi, so on the
shallow shapes five trajectories reach the levels 8 and past 12 only where few wires jump: there `hot` wires (HOT_WIRES) keep
their t1 and the others' is 200 times as long.  A case's LEVEL is the largest log10 of a wire's
product of 1 / sqrt(1 - gamma) since the last fired site that any of its trajectories meets on the way back
(device_traj_grad_reference.walk: 'level'); it depends on the pattern that fires, so (tau, seed, row0) of JUMP were found by
scanning seeds with grad=False walks on the CPU.  tests/test_traj_precision_oracle.py asserts every level.
"""
import zlib
from collections import namedtuple

import numpy as np

from oracle import hea_oracle as O
from oracle.ld_oracle import err
from tests import device_traj_grad_reference as G
from tests import noise_oracle as NO
from tests import noisy_traj_grad_reference as NTG
from tests.density_precision_cases import _is, quantities, split
from tests.noise_oracle import WIDE, real_of as NO_real_of
from tests.precision_cases import FACTOR, ULP, Reference, budget, e_ref, measure, _maxabs        # noqa: F401 (the rule)

assert np.finfo(np.longdouble).nmant >= 63, 'np.longdouble is not wider than float64 here: no reference for these budgets'

T = 5
SEED0 = 3600
HAM_BOUND = (-5.0, 5.0)
README_RATES = (1e-3, 1e-2)
HEAVY_RATES = (0.05, 0.1)
READOUT = 0.01
QUANTITIES = ('row', 'sse', 'pred')
SHAPES = ((7, (10, 2)), (9, (3, 2)), (10, (6, 2)), (12, (2, 2)))
KERNEL = {('sampled', False): 'noisy_grad_wave_kernel', ('sampled', True): 'noisy_grad_lds_kernel',
          ('jump', False): 'device_grad_wave_kernel', ('jump', True): 'device_grad_lds_kernel'}
# level name -> the window its case's LEVEL must lie in
LEVELS = {'low': (0.0, 1.0), 'L2': (1.5, 2.5), 'L4': (3.5, 4.5), 'L8': (7.5, 8.5), 'past12': (12.0, np.inf)}

Case = namedtuple('Case', 'id family n kind net readout rows rates level tau polar seed row0 hot')
# family: 'sampled' | 'jump'.  kind / net: 'heaqnn' (blocks, LD) or 'quanonet' (branch depth, LD, trunk depth, LD).  rates: the
# sampled family's (p1, p2).  level: a key of LEVELS, or None (the polar and the rescale case: their LEVEL is printed).  tau:
# the jump family's durations.  polar: X / Y errors of 0.3 .. 0.4 in front of the relaxation.  seed, row0: of the random stream.
# hot: 0, or the number of wires that keep their t1 while the others' is 200 times as long (see the head of the file).

# id -> (tau, sampling seed, row0, hot): see the head of the file
JUMP = {'jump-q7-10x2-low': (0.004, 40, 0, 0), 'jump-q7-10x2-L2': (1.207, 40, 0, 0), 'jump-q7-10x2-L4': (4.48, 40, 0, 0),
        'jump-q7-10x2-L8': (5.825, 46, 0, 0),
        'jump-q9-3x2-low': (0.004, 40, 0, 0), 'jump-q9-3x2-L2': (2.039, 40, 0, 0), 'jump-q9-3x2-L4': (5.825, 40, 0, 0),
        'jump-q9-3x2-L8': (7.572, 40, 0, 2), 'jump-q9-3x2-past12': (12.796, 41, 0, 2),
        'jump-q10-6x2-low': (0.004, 40, 0, 0), 'jump-q10-6x2-L2': (2.039, 40, 0, 0), 'jump-q10-6x2-L4': (5.825, 40, 0, 0),
        'jump-q10-6x2-L8': (5.825, 40, 0, 2), 'jump-q10-6x2-past12': (16.635, 40, 0, 2),
        'jump-q12-2x2-low': (0.004, 40, 0, 0), 'jump-q12-2x2-L2': (2.039, 40, 0, 0), 'jump-q12-2x2-L4': (5.825, 40, 0, 0),
        'jump-q12-2x2-L8': (7.572, 44, 0, 2), 'jump-q12-2x2-past12': (21.626, 42, 0, 2),
        'jump-q9-3x2-polar': (0.5, 40, (1 << 32) + 5, 0), 'jump-q7-20x2-rescale': (7.0, 40, 3, 0)}

# id of a planned case -> (its planned level, the level used, why): a case whose references alone cannot meet
# budget(row) <= 2^-10 max|row_ld| at the planned level.  Measured with the references alone, printed by
# tests/test_traj_precision_oracle.py (test_inverse_walk_without_restart_leaves_the_budget_past_12).
LOWERED = {'jump-q7-10x2-past12': ('past12', 'L8', 'at LEVEL 12.05 (tau 12.796, seed 42) the fp64 inverse walk is 4.7e+4 off on a largest '
                                                  'entry of 61: e_ref itself is wrong in every digit; jump-q7-10x2-L8 (8.23) is the level '
                                                  'that runs.  quanonet_amd.noise refuses the setting (JUMP_GAMMA_MAX)')}
# the planned case all the same: what the finding is stated on (never run on a GPU)
PAST12_Q7 = ('jump-q7-10x2-past12', 12.796, 42, 0, 0)

# id -> seed of the case's model and rows, where the default (from the case's id) breaks a condition on the inputs that
# tests/test_traj_precision_oracle.py states
SEEDS = {'jump-q12-2x2-low': 1001}        # the default's y lies within |pred| / 8 of pred (0.166 against 0.183)


# the sampled family: id -> (n, kind, net, read-out, rows, rates, sampling seed, row0).  The README's rates at the four shapes,
# the heavy setting at n = 7 and n = 10; the n = 9 case is the trainable-frequency QuanONet (2 + 1 blocks of LD 2)
SAMPLED = {'sampled-q7-10x2': (7, 'heaqnn', (10, 2), 'Z', 2, README_RATES, 40, 0),
           'sampled-q7-10x2-heavy': (7, 'heaqnn', (10, 2), 'X', 2, HEAVY_RATES, 41, 3),
           'sampled-q9-net2212': (9, 'quanonet', (2, 2, 1, 2), 'Y', 2, README_RATES, 40, 0),
           'sampled-q10-6x2': (10, 'heaqnn', (6, 2), 'diag', 2, README_RATES, 40, 0),
           'sampled-q10-6x2-heavy': (10, 'heaqnn', (6, 2), 'Z', 2, HEAVY_RATES, 41, (1 << 32) + 1),
           'sampled-q12-2x2': (12, 'heaqnn', (2, 2), 'X', 1, README_RATES, 40, 0)}
SHIFTED_ANGLES = 16                   # angles per sampled case at which the fp64 shift is evaluated (_shift_form)


def _cases():
    out = [Case(cid, 'sampled', n, kind, net, readout, rows, rates, None, None, False, seed, row0, 0)
           for cid, (n, kind, net, readout, rows, rates, seed, row0) in SAMPLED.items()]
    spread = {7: 'Z', 9: 'Y', 10: 'diag', 12: 'X'}
    for n, net in SHAPES:
        for level in LEVELS:
            cid = f'jump-q{n}-{net[0]}x{net[1]}-{level}'
            if cid not in LOWERED:
                tau, seed, row0, hot = JUMP[cid]
                out.append(Case(cid, 'jump', n, 'heaqnn', net, spread[n], 1, README_RATES, level, tau, False, seed, row0, hot))
    for cid, n, net, readout, polar in (('jump-q9-3x2-polar', 9, (3, 2), 'X', True), ('jump-q7-20x2-rescale', 7, (20, 2), 'Z', False)):
        tau, seed, row0, hot = JUMP[cid]
        out.append(Case(cid, 'jump', n, 'heaqnn', net, readout, 1, README_RATES, None, tau, polar, seed, row0, hot))
    return out


def past12_q7():
    """the lowered past-12 case as planned"""
    cid, tau, seed, row0, hot = PAST12_Q7
    return Case(cid, 'jump', 7, 'heaqnn', (10, 2), 'Z', 1, README_RATES, 'past12', tau, False, seed, row0, hot)


CASES = _cases()


def cfgs_of(case):
    return (O.block_configs_quanonet if case.kind == 'quanonet' else O.block_configs_heaqnn)(case.n, case.net)


def jump_setting(n, tau, polar=False, level=None, hot=0, seed=0):
    """the DeviceNoise of a jump case (the head of the file)"""
    from quanonet_amd.noise import DeviceNoise
    rng = np.random.default_rng(3600 + 10 * n + seed)
    t1 = rng.uniform(0.8, 1.4, n)
    if hot:
        t1[[q for q in range(n) if q not in HOT_WIRES(n)[:hot]]] *= 200.0
    p1, p2 = (rng.uniform(0.3, 0.4, n), rng.uniform(0.3, 0.4, n)) if polar else README_RATES
    return DeviceNoise(p1=p1, p2=p2, readout01=rng.uniform(0.01, 0.05, n), readout10=rng.uniform(0.04, 0.09, n), t1=t1, t2=t1,
                       t_rx=tau, t_rot=tau, t_cx=tau, idle=level == 'low')


def HOT_WIRES(n):
    """the wires that stay short-lived in a `hot` setting, in order: one that a lane bit selects, one that a register or an
    LDS pass selects (q >= 6), then the middle one"""
    return [1, n - 1, n // 2]


def as_dict(dn, n):
    d = {k: [dn._at(k, q) for q in range(n)] for k in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2')}
    d.update(t_rx=dn.t_rx, t_rot=dn.t_rot, t_cx=dn.t_cx, idle=dn.idle)
    return d


def _seed(case):
    """of the case's model and rows: from its id, so that a case keeps its circuit when the table around it changes"""
    return SEED0 + SEEDS.get(case.id, zlib.crc32(case.id.encode()) % 1000)


_INPUTS = {}
Inputs = namedtuple('Inputs', 'model flat ins y noise sampling nz')
# model: the fp64 torch model on the CPU.  ins: (x,) or (branch, trunk).  noise: quanonet_amd.noise.NoiseModel with T and the
# seed (sampled) or DeviceNoise (jump); sampling: None or the jump family's Sampling; nz: None or the jump setting as a dict.


def inputs_of(case):
    """the case's model, rows and noise setting, made once"""
    if case.id in _INPUTS:
        return _INPUTS[case.id]
    import torch
    from quanonet_amd.noise import NoiseModel, Sampling
    from tests import helpers as H
    n, seed = case.n, _seed(case)
    rng = np.random.default_rng(seed)
    kw = dict(ham_bound=HAM_BOUND)
    if case.readout == 'diag':
        diag = rng.normal(size=1 << n)
        kw['ham_diag'] = diag - diag.mean()
    else:
        kw['ham_pauli'] = case.readout
    if case.kind == 'quanonet':
        m = H.quanonet(n, 6, 2, case.net, seed - SEED0, if_trainable_freq=True, scale_coeff=np.pi, **kw)
        ins = (rng.uniform(-1, 1, (case.rows, 6)), rng.uniform(-1, 1, (case.rows, 2)))
    else:
        m = H.heaqnn(n, n * case.net[0], case.net, seed - SEED0, if_trainable_freq=False, scale_coeff=np.pi, **kw)
        ins = (rng.uniform(-1, 1, (case.rows, n * case.net[0])),)
    with torch.no_grad():
        w = m.quantum_layer.ansatz_weights
        w.copy_(torch.from_numpy(rng.uniform(-np.pi, np.pi, tuple(w.shape))))
    y = rng.normal(scale=0.7, size=case.rows)
    if case.family == 'sampled':
        noise = NoiseModel(p1=case.rates[0], p2=case.rates[1], readout=READOUT, trajectories=T, seed=case.seed)
        sampling = nz = None
    else:
        noise = jump_setting(n, case.tau, case.polar, case.level, case.hot)
        sampling, nz = Sampling(trajectories=T, seed=case.seed), as_dict(noise, n)
    _INPUTS[case.id] = Inputs(m, H.flat(m).numpy(), ins, y, noise, sampling, nz)
    return _INPUTS[case.id]


def circuit_of(case):
    """(x[rows, E], w[blk, 3, n], read-out keywords) of the case's circuit in float64: what the walks below see of the model"""
    import torch
    from tests.test_noisy_forward import _circuit
    i = inputs_of(case)
    c, _ = _circuit(i.model, tuple(torch.as_tensor(t) for t in i.ins))
    return c['x'], c['w'], dict(offset=c['offset'], coeff=c['coeff'], ham_diag=c['ham_diag'], ham_pauli=c['ham_pauli'])


def pattern_walk(case, **kw):
    """device_traj_grad_reference.walk of a jump case's circuit without the gradient: pattern, margins, level, counts"""
    i = inputs_of(case)
    x, w, ro = circuit_of(case)
    return G.walk(case.n, cfgs_of(case), x, w, i.nz, T, case.seed, row0=case.row0, grad=False, **ro, **kw)


def _shift_form(n, cfgs, x, w, noise, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', row0=0, dtype=np.complex128):
    """The second fp64 evaluation of the sampled family: noisy_traj_grad_reference.traj_grad_shift's rule -- central differences
    at +- pi / 2 of noise_oracle.replay_values on the same stream, the value from the unshifted replay -- at SHIFTED_ANGLES of
    the circuit's angles, evenly spread over the encoding and the ansatz angles in their order; the other entries are the
    adjoint walk's.  A full shift replays the circuit twice per angle (980 replays at n = 7, 10 x LD 2: 24 s; 40 s at n = 10,
    6 x LD 2), which the CPU file's run time does not hold at the depths that are trained.  e_ref is a maximum over entries, so
    leaving shifted entries out can only lower it: a budget made this way is never wider than the full shift's.  The read-out
    weights are made once (a diagonal read-out's fold has 4^n terms)."""
    real = NO_real_of(dtype)
    weights = NTG.readout_weights(n, offset, coeff, ham_diag, float(noise.readout), real)
    x, w = np.asarray(x, real), np.asarray(w, real)
    val = lambda xx, ww: NO.replay_values(n, cfgs, xx, ww, noise, offset, coeff, ham_diag, ham_pauli, row0, dtype, weights).mean(axis=1)
    _, gx, gw = NTG.traj_grad(n, cfgs, x, w, noise, offset, coeff, ham_diag, ham_pauli, row0, dtype)
    gx, gw = gx.copy(), gw.copy()
    slots = [(0, e) for e in range(x.shape[1])] + [(1, idx) for idx in np.ndindex(w.shape)]
    hp = NTG.half_pi(real)
    for which, at in slots[::-(-len(slots) // SHIFTED_ANGLES)]:
        d = [np.zeros_like(x), np.zeros_like(w)]
        d[which][(slice(None), at) if which == 0 else at] = hp
        g = 0.5 * (val(x + d[0], w + d[1]) - val(x - d[0], w - d[1]))
        if which == 0:
            gx[:, at] = g
        else:
            gw[(slice(None),) + at] = g
    return val(x, w), gx, gw


def walk(case, form='adjoint', dtype=np.complex128, restart_above=G.RESTART_ABOVE):
    """([P + 2] buffer, pred[rows]) of the case through the numpy model.  form: sampled family 'adjoint' | 'shift'; jump family
    'stored' | 'inverse' (with restart_above; None: no restart)"""
    i = inputs_of(case)
    if case.family == 'sampled':
        engine = NTG.TrajEngine(i.noise, case.row0, {'adjoint': NTG.traj_grad, 'shift': _shift_form}[form], dtype=dtype)
    else:
        kw = dict(inverse=True, restart_above=restart_above) if form == 'inverse' else {}
        if np.dtype(dtype) != np.complex128:
            kw['dtype'] = dtype
        engine = G.DeviceTrajEngine(i.nz, T, case.seed, case.row0, **kw)
    return NTG.model_loss_grad(i.model, i.ins, i.y, 1.0 / case.rows, engine, dtype=dtype)


_REFS = {}


def reference(case):
    """Reference (tests/precision_cases.py) of one case, computed once per process: ld = the wide adjoint / stored walk as
    (hi, lo) pairs, e_c = the fp64 adjoint / stored walk's error against it, e_np = the fp64 shift's / inverse walk's"""
    if case.id not in _REFS:
        first, second = ('adjoint', 'shift') if case.family == 'sampled' else ('stored', 'inverse')
        ld = {q: split(v) for q, v in quantities(*walk(case, first, dtype=WIDE)).items()}
        errs = []
        for form in (first, second):
            got = quantities(*walk(case, form))
            errs.append({q: _maxabs(err(got[q], ld[q])) for q in QUANTITIES})
        for pair in ld.values():
            for a in pair:
                a.setflags(write=False)
        _REFS[case.id] = Reference(inputs_of(case), ld, errs[0], errs[1])
    return _REFS[case.id]


# ---------------------------------------------------------------------------------------------------------------------
# the code under test (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def run_case(dev, case):
    """The case's one loss_grad call on the device: ({'row', 'sse', 'pred'}, the kernel's mangled name).  The kernel is asserted
    by name to be the case's unit's, instantiated for the case's n, so that a budget is never credited to another kernel."""
    import torch
    from quanonet_amd import _lib
    from tests.helpers import kernel_launches, mangled_is
    i = inputs_of(case)
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    desc = i.model.fused_desc()
    flat, y = t(i.flat), t(i.y)
    branch, trunk = t(i.ins[0]), t(i.ins[1] if len(i.ins) > 1 else None)
    q = i.model.quantum_layer
    diag = q.ham_diag.to(dev) if q.use_full_ham else None
    grad = torch.full((flat.numel() + 2,), float('nan'), dtype=torch.float64, device=dev)
    pred = torch.full((case.rows,), float('nan'), dtype=torch.float64, device=dev)
    lds = case.n >= 10
    if case.family == 'sampled':
        entry = _lib.model_loss_grad_noisy_lds if lds else _lib.model_loss_grad_noisy_wide
        recs = (i.noise.params(),)
    else:
        entry = _lib.model_loss_grad_noisy_device_lds if lds else _lib.model_loss_grad_noisy_device
        recs = (i.noise.params(case.n), i.sampling.params())

    def call():
        entry(desc, branch, trunk, y, flat, *recs, 1.0 / case.rows, grad, row0=case.row0, ham_diag=diag, pred=pred)
    call()
    _lib.check_status(dev)
    torch.cuda.synchronize()
    got = quantities(grad.cpu().numpy(), pred.cpu().numpy())
    launches = kernel_launches(dev, call)
    _lib.check_status(dev)
    hits = [name for name, _, _ in launches for ident in KERNEL.values() if _is(mangled_is, name, ident)]
    assert len(hits) == 1, [l[0] for l in launches]
    assert _is(mangled_is, hits[0], KERNEL[case.family, lds], (case.n,)), (hits[0], KERNEL[case.family, lds], case.n)
    return got, hits[0]
