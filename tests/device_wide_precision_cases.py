"""
Error budgets of the exact forward under a device noise model at n = 7, 8, 9: the kernel chain of hea_density_device_wide.hip
(density_dev_wide_ring_kernel, density_dev_wide_wires_kernel, density_dev_wide_values_kernel and the shared read-out kernel).
Test infrastructure; importing it needs no GPU.  tests/test_device_wide_precision_oracle.py (CPU) checks the references and the
condition on the inputs, tests/test_device_wide_precision_budget.py (GPU) the kernels.

Everything but the table is tests/forward_precision_cases.py's, by import: the rule budget(q) = 32 x max(e_ref(q), 2^-53 scale(q)),
Reference, reference, measure, scale, and the device family's references -- q_ld the Kraus timeline of
device_noise_reference.final_rho in np.clongdouble, e_ref the larger error of that timeline in complex128 and of the stored walk's
forward sweep (device_noise_grad_reference.stored_final_rho) read out the way the kernels do it.  A case here is a Case of that
module with family 'device', so its references are that family's.  Two things of that module are keyed by its own table and are
filled from here, into the caches it looks in first: the inputs of a case (inputs_of below, made the same way from this table's
seeds) and the outcome probabilities of a case (probabilities below: that module's _probabilities for the device family, with
this table's pairs of cases that share one evolution, SHARED).  Its own table and SHARED are left as they are.  The entry points
for a case of this table are therefore reference_of, inputs_of, probabilities and run_case below, which fill those caches before
that module looks; forward_precision_cases.reference called directly on such a case finds nothing and raises on its own table's
index.  A hook in that module taking the table, the seeds and the setting would be the sturdier form; it is a change to that
module.

Rows: two at n = 7, 8 (row 1 shows rho + (r << 2N) and csr), one at n = 9, as for the uniform chain.  Noise: perwire_setting
below, no two wires and no two ring slots alike: forward_precision_cases.perwire_setting, whose p2 repeats at n = 8 (slots 1 and
6, 2 and 7), with another slope on p2 there.  Cost: the long-double timeline at n = 9 and (3, 2) takes a minute of numpy, once
for the Z and the X case.

Lowered: none.  The condition budget(q) <= CAP = 1e-12 holds at the planned depths (figures: the CPU file prints them).
"""
import numpy as np

from tests import forward_precision_cases as FP
from tests.forward_precision_cases import CAP, QUANTITIES, Case, budget, measure, reference, scale    # noqa: F401 (the machinery)

SEED0 = 3900
KERNELS = ('density_dev_wide_ring_kernel', 'density_dev_wide_wires_kernel', 'density_wide_readout_kernel',
           'density_dev_wide_values_kernel')
LOWERED = {}
# id -> the id of the case whose circuit, row and noise it shares; only the read-out basis differs
SHARED = {'device-wide-q9-3x2-perwire-X': 'device-wide-q9-3x2-perwire'}


def _cases():
    out = []

    def add(n, net, readout, noise, kind='heaqnn'):
        blocks = net[0] if kind == 'heaqnn' else net[0] + net[2]
        cid = f'device-wide-q{n}-{blocks}x{net[1]}-{noise}' + ('' if readout == 'Z' else f'-{readout}')
        out.append(Case(cid, 'device', n, kind, net, readout, noise, 1 if n == 9 else 2))

    for n, readout in ((7, 'Z'), (8, 'diag'), (9, 'Z')):
        add(n, (3, 2), readout, 'perwire')
    add(7, (3, 2), 'Y', 'perwire-noidle')
    add(9, (3, 2), 'X', 'perwire')
    add(8, (2, 0), 'Z', 'perwire')                                       # stage B serves exactly one pair: dev_wide_wire_pass<8, 1, 4>
    return out


CASES = _cases()
_EVOLVED = {}


def perwire_setting(n, idle=True):
    """forward_precision_cases.perwire_setting where no two of its ring slots agree (n = 7, 9 and every n <= 6); elsewhere the
    same setting with p2[q] = 5e-3 (2 + 3 q mod n) + 1.7e-3 q"""
    import dataclasses
    dn = FP.perwire_setting(n, idle)
    if len(set(dn.p2)) < n:
        dn = dataclasses.replace(dn, p2=tuple(5e-3 * (2 + (3 * q) % n) + 1.7e-3 * q for q in range(n)))
    for name in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2'):
        assert len(set(getattr(dn, name))) == n, (name, n)
    return dn


def inputs_of(case):
    """forward_precision_cases.inputs_of for a case of this table: the same models, rows and settings from this table's seeds"""
    if case.id not in FP._INPUTS:
        import torch
        from tests import density_grad_reference as DG
        from tests import helpers as H
        n = case.n
        seed = SEED0 + [c.id for c in CASES].index(SHARED.get(case.id, case.id))
        rng = np.random.default_rng(seed)
        kw = dict(scale_coeff=np.pi, ham_bound=FP.HAM_BOUND)
        if case.readout == 'diag':
            diag = rng.normal(size=1 << n)
            kw['ham_diag'] = diag - diag.mean()
        else:
            kw['ham_pauli'] = case.readout
        assert case.kind == 'heaqnn'
        m = H.heaqnn(n, n * case.net[0], case.net, seed - SEED0, if_trainable_freq=case.net[1] == 0, **kw)
        branch = rng.uniform(-1, 1, (case.rows, n * case.net[0]))
        with torch.no_grad():
            w = m.quantum_layer.ansatz_weights
            w.copy_(torch.from_numpy(rng.uniform(-np.pi, np.pi, tuple(w.shape))))
        noise = perwire_setting(n, idle=case.noise == 'perwire')
        FP._INPUTS[case.id] = FP.Inputs(m, DG.spec_of(m), H.flat(m).numpy(), branch, None, noise)
    return FP._INPUTS[case.id]


def probabilities(case, form, dtype=np.complex128):
    """forward_precision_cases.probabilities for a case of this table: (diag rho [rows, 2^n], the bias), once per process.  form
    'channel' is the Kraus timeline, 'second' the stored walk's forward sweep; the evolution ends in the Z basis and the basis
    change of the case follows, each form with its own, so that the cases of SHARED evolve once"""
    from tests import density_grad_reference as DG
    from tests import density_reference as DR
    key = (case.id, form, np.dtype(dtype))
    if key not in FP._PROBS:
        i = inputs_of(case)
        mc = DG.model_circuit(i.spec, i.flat, i.branch, i.trunk, dtype)
        n, D = mc.n, 1 << mc.n
        ekey = (SHARED.get(case.id, case.id), form, np.dtype(dtype))
        if ekey in _EVOLVED:
            rho = _EVOLVED[ekey]
        else:
            rho_of = FP.DNR.final_rho if form == 'channel' else FP.DV.stored_final_rho
            rho = rho_of(n, mc.cfgs, mc.x, mc.w, FP.noise_dict(case), 'Z', dtype)
            if ekey[0] in SHARED.values():
                _EVOLVED[ekey] = rho
        change = FP.DNR.basis_change if form == 'channel' else DR.basis_change
        rho = np.ascontiguousarray(change(rho.reshape((-1,) + (2,) * (2 * n)), n, i.spec['ham_pauli'])).reshape(-1, D, D)
        prob = np.real(np.einsum('bkk->bk', rho)).copy()
        prob.setflags(write=False)
        FP._PROBS[key] = (prob, mc.flat[0] if mc.quanonet else DR.real_of(dtype)(0.0))
    return FP._PROBS[key]


def reference_of(case):
    """forward_precision_cases.reference of a case of this table"""
    for form, dtype in (('channel', FP.WIDE), ('channel', np.complex128), ('second', np.complex128)):
        probabilities(case, form, dtype)
    return reference(case)


def run_case(dev, case):
    """The case's one forward call on the device: ({'pred', 'sd'}, the mangled names of the unit's kernels that ran), asserted
    by name and first template argument to be the case's: the stage kernels its circuit needs, one value-table and one read-out
    kernel, all at n, and neither the n <= 6 kernels nor the uniform chain's stages."""
    import torch
    from quanonet_amd import _lib
    from tests.density_precision_cases import _is
    from tests.helpers import kernel_launches, mangled_is
    i = inputs_of(case)
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    desc = i.model.fused_desc()
    flat, branch, trunk = t(i.flat), t(i.branch), t(i.trunk)
    q = i.model.quantum_layer
    diag = q.ham_diag.to(dev) if q.use_full_ham else None
    pred = torch.full((case.rows,), float('nan'), dtype=torch.float64, device=dev)
    sd = torch.full((case.rows,), float('nan'), dtype=torch.float64, device=dev)
    rec = i.noise.params(case.n)

    def call():
        _lib.model_forward_noisy_device_exact_wide(desc, branch, trunk, flat, rec, ham_diag=diag, out=pred, shot_std=sd)
    call()
    _lib.check_status(dev)
    torch.cuda.synchronize()
    got = {'pred': pred.cpu().numpy(), 'sd': sd.cpu().numpy()}
    names = [k[0] for k in kernel_launches(dev, call)]
    _lib.check_status(dev)
    other = [k for k in names for ident in tuple(FP.KERNEL.values()) + FP.WIDE_KERNELS[:2] if _is(mangled_is, k, ident)]
    assert not other, names
    ring, wires, readout, values = ([k for k in names if _is(mangled_is, k, ident)] for ident in KERNELS)
    cfgs = FP.cfgs_of(case)
    sublayers, ld0 = sum(ld for _, ld in cfgs), sum(ld == 0 for _, ld in cfgs)
    assert len(ring) == 2 * sublayers and len(wires) == 2 * ld0 + (2 if case.readout in ('X', 'Y') else 0), names
    assert len(readout) == 1 and len(values) == 1, names
    for k, ident in [(k, KERNELS[0]) for k in ring] + [(k, KERNELS[1]) for k in wires] + [(readout[0], KERNELS[2]),
                                                                                            (values[0], KERNELS[3])]:
        assert _is(mangled_is, k, ident, (case.n,)), (k, ident, case.n)
    return got, sorted(set(ring + wires + readout + values))
