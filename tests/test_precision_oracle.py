"""
The long-double oracle (oracle/ld_oracle.py) and the case table of the error budgets (tests/precision_cases.py).  CPU only.

* it agrees with the fp64 C oracle to 1e-12 on every case of the table, its hi part reproduces the known answers K1-K8 that
  tests/test_oracle_golden.py pins, and inside it the adjoint gradient equals the parameter-shift rule to 1e-17 x scale
  (exact rational arithmetic on the (hi, lo) pairs, angles theta +- pi/2 given with their low parts);
* condition on the inputs: on every case and quantity each fp64 oracle's error is within 8 times the other's;
* every budget is at most 1e-11;
* the kernels the table names are AUTO's own where the case runs under AUTO (tests/test_dispatch_regimes.py: expected).

The sample counts that follow the device (2 CUs + 1, ...) are taken at 256 CUs here.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import hea_oracle as O
from oracle import c_oracle as C
from oracle import ld_oracle as L
from tests import helpers as H
from tests import precision_cases as PC

CUS = PC.CUS_NOMINAL
CIRCUIT_Q = ('out', 'state', 'grad_x', 'grad_w')
MODEL_Q = ('row', 'sse', 'out')
ALL_CASES = [(c, CIRCUIT_Q) for c in PC.CIRCUIT_CASES] + [(c, MODEL_Q) for c in PC.MODEL_CASES]
IDS = [c.id for c, _ in ALL_CASES]


def _reference(case):
    return PC.model_reference(case) if isinstance(case, PC.ModelCase) else PC.circuit_reference(case, case.batch(CUS))


def test_table_ids_are_unique_and_every_family_has_a_random_case():
    assert len(set(IDS)) == len(IDS)
    families = {c.id.rsplit('-', 1)[0] for c in PC.CIRCUIT_CASES}
    assert families == {c.id.rsplit('-', 1)[0] for c in PC.CIRCUIT_CASES if c.inputs == 'random'}


@pytest.mark.parametrize('case,quantities', ALL_CASES, ids=IDS)
def test_long_double_oracle_agrees_with_the_c_oracle(case, quantities):
    ref = _reference(case)
    for q in quantities:
        assert np.isfinite(ref.ld[q][0]).all() and np.isfinite(ref.ld[q][1]).all(), q
        assert ref.e_c[q] <= 1e-12, (q, ref.e_c[q])
        hi, lo = ref.ld[q]
        assert (np.abs(lo) <= np.spacing(np.abs(hi))).all(), q                # lo is what hi leaves over


@pytest.mark.parametrize('case,quantities', ALL_CASES, ids=IDS)
def test_each_fp64_oracle_is_within_8x_of_the_other(case, quantities):
    """the condition on the inputs: a seed on which one oracle is lucky would make e_ref say little (change the seed then)"""
    ref = _reference(case)
    for q in quantities:
        a, b = ref.e_c[q], ref.e_np[q]
        assert max(a, b) <= 8 * min(a, b), (q, a, b)


@pytest.mark.parametrize('case,quantities', ALL_CASES, ids=IDS)
def test_every_budget_is_at_most_1e_11(case, quantities):
    ref = _reference(case)
    for q in quantities:
        assert PC.budget(ref, q) <= 1e-11, (q, PC.e_ref(ref, q), PC.budget(ref, q))


@pytest.mark.parametrize('case', [c for c in PC.CIRCUIT_CASES if c.variant == 'auto'], ids=lambda c: c.id)
def test_kernels_named_by_the_table_are_the_automatic_choice(case):
    pauli = 'Z' if case.readout == 'diag' else case.readout
    want = PC.expected(case.n, case.cfgs, case.batch(CUS), CUS, pauli)
    assert (case.fwd[0], case.bwd[0]) == (want.fwd, want.bwd), want
    if case.bwd[0] == 'bwd_ztri_kernel':
        assert case.bwd[1] == (case.n, want.pipes)
    if case.bwd[0] == 'bwd_kernel':
        assert (case.bwd[1] == (case.n, 2)) == want.dense


def test_wide_set_sits_on_both_sides_of_the_half_angle_switch():
    case = next(c for c in PC.CIRCUIT_CASES if c.inputs == 'wide')
    x = PC.circuit_inputs(case, 3)[0]
    half = np.abs(0.5 * x).reshape(-1)
    assert (half[::7] >= 1e5).any() and ((half[::7] < 1e5) & (half[::7] > 9.9e4)).any()
    assert (np.delete(half, np.arange(0, half.size, 7)) <= 500).all()
    assert {float(v) for v in x.reshape(-1)[::7]} == set(PC.WIDE_SPECIAL)


# ---------------------------------------------------------------------------------------------------------------------
# the known answers K1-K8 (tests/test_oracle_golden.py), on the hi part
# ---------------------------------------------------------------------------------------------------------------------
def test_k1_k2_antiderivative_analytic():
    p = H.load_pt_params('antideriv_q2.npz', 2, (5, 1, 5, 1))
    trunk = np.linspace(0, 1, 100)[:, None]
    ka = H.known_answers()
    off, co = O.ham_params(2, -5.0, 5.0)
    cfgs = O.block_configs_quanonet(2, (5, 1, 5, 1))
    for key, bv, truth in [('K1', np.cos(np.pi * np.linspace(0, 1, 10)), np.sin(np.pi * trunk[:, 0]) / np.pi),
                           ('K2', np.linspace(0, 1, 10), 0.5 * trunk[:, 0] ** 2)]:
        x = H.encode_quanonet(p, np.tile(bv, (100, 1)), trunk)
        out = L.hea_forward(2, cfgs, x, p['quantum_layer.ansatz_weights'], off, co)[0] + p['bias'][0]
        rel = np.linalg.norm(out - truth) / np.linalg.norm(truth)
        assert rel < ka[key]['rel_l2_max']
        assert abs(rel - ka[key]['survey_rel_l2']) < 2e-3


@pytest.mark.parametrize('key,op,tag,npts', H.PDE_CASES)
def test_k3_k8_notebook_figures(key, op, tag, npts):
    ka = H.known_answers()[key]
    p = H.load_pt_params(f'{op}_q5.npz', 5, (40, 2, 20, 2))
    branch, trunk = H.notebook_inputs(npts, H.U0[tag])
    x = H.encode_quanonet(p, branch, trunk)
    off, co = O.ham_params(5, -5.0, 5.0)
    cfgs = O.block_configs_quanonet(5, (40, 2, 20, 2))
    out = L.hea_forward(5, cfgs, x, p['quantum_layer.ansatz_weights'], off, co)[0] + p['bias'][0]
    truth = np.load(H.GOLDEN + '/pde_truths.npz')[f'{op}_{tag}']
    diff = truth - out.reshape(npts, npts)
    assert H.fmt1e(np.mean(diff ** 2)) == ka['mse']
    assert H.fmt1e(np.mean(np.abs(diff))) == ka['mae']


# ---------------------------------------------------------------------------------------------------------------------
# the reference's gradient is right in its own precision
# ---------------------------------------------------------------------------------------------------------------------
PI_2_HI = 0.5 * np.pi
PI_2_LO = 6.123233995736766e-17              # pi / 2 - PI_2_HI


def _exact(pair):
    hi, lo = pair
    return [Fraction(float(h)) + Fraction(float(l)) for h, l in zip(np.ravel(hi), np.ravel(lo))]


def _shifted(a, idx, sign):
    """a with a[idx] + sign pi/2 as (hi, lo): the float64 sum, and what it leaves of the exact one to 1e-33"""
    hi, lo = np.array(a, np.float64), np.zeros_like(a, dtype=np.float64)
    exact = Fraction(float(a[idx])) + sign * (Fraction(PI_2_HI) + Fraction(PI_2_LO))
    hi[idx] = float(exact)
    lo[idx] = float(exact - Fraction(float(hi[idx])))
    return hi, lo


def test_adjoint_equals_parameter_shift_inside_the_long_double_oracle():
    n, cfgs, B = 3, [(3, 1), (2, 2)], 4
    rng = np.random.default_rng(11)
    E, blk = O.circuit_sizes(n, cfgs)
    x, w, g = rng.uniform(-np.pi, np.pi, (B, E)), rng.uniform(-np.pi, np.pi, (blk, 3, n)), rng.normal(size=B)
    off, co = O.ham_params(n, *PC.HAM_BOUND)
    _, gx, gw = L.hea_backward(n, cfgs, x, w, g, off, co)
    gx_exact, gw_exact = np.array(_exact(gx), dtype=object).reshape(B, E), np.array(_exact(gw), dtype=object).reshape(w.shape)
    gq = [Fraction(float(v)) for v in g]
    scale = max(1.0, float(np.abs(gw[0]).max()), float(np.abs(gx[0]).max()))
    for idx in [(0, 0, 0), (blk - 1, 2, n - 1), (blk // 2, 1, n // 2)]:
        f = []
        for sign in (1, -1):
            hi, lo = _shifted(w, idx, sign)
            f.append(_exact(L.hea_forward(n, cfgs, x, hi, off, co, w_lo=lo)))
        ps = sum(gb * (fp - fm) / 2 for gb, fp, fm in zip(gq, *f))
        assert abs(float(ps - gw_exact[idx])) <= 1e-17 * scale, (idx, float(ps - gw_exact[idx]))
    for col in (0, E - 1, E // 2):
        f = []
        for sign in (1, -1):
            his, los = zip(*[_shifted(x[b], col, sign) for b in range(B)])
            f.append(_exact(L.hea_forward(n, cfgs, np.stack(his), w, off, co, x_lo=np.stack(los))))
        for b in range(B):
            d = float(gq[b] * (f[0][b] - f[1][b]) / 2 - gx_exact[b, col])
            assert abs(d) <= 1e-17 * scale, (col, b, d)


def test_model_level_chain_rule_matches_the_fp64_oracle_per_parameter():
    """the C model-level routine against hea_oracle.quanonet_loss_and_grads, name by name (layout of the frequency gradients)"""
    case = PC.MODEL_CASES[0]
    m, cfgs, (branch, trunk, y) = PC.model_of(case)
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    for bt in (None, 212):
        sse, grads, out = L.quanonet_loss_and_grads(sd, branch, trunk, y, case.n, case.net, batch_total=bt)
        loss, want, wout = O.quanonet_loss_and_grads(sd, branch, trunk, y, case.n, case.net, batch_total=bt, engine=C)
        assert set(grads) == set(want)
        for k in want:
            np.testing.assert_allclose(grads[k][0].reshape(-1), np.asarray(want[k]).reshape(-1), rtol=0, atol=1e-12, err_msg=k)
        np.testing.assert_allclose(out[0], wout, rtol=0, atol=1e-12)
        assert abs(sse[0] / (bt or len(y)) - loss) <= 1e-12
