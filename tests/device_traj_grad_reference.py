"""
numpy reference for the quantum-jump trajectory gradient under the device noise model (qhea_model_loss_grad_noisy_device,
include/quanonet_hea.h).

walk replays the stream of tests/device_traj_reference.py replay_values gate by gate with the KERNEL's rule: the state stays
unnormalised, a damping site on wire q jumps iff u N2 < gamma M (N2 the state's squared norm, M the part of it with the wire in
|1>), a jump applies L = |0><1|, no jump K0 = diag(1, sqrt(1 - gamma)), and a segment whose N2 ends below 2^-200 is rescaled by
2^100.  It records the pattern that fired (and with `forced` replays a recorded pattern instead of deciding), keeps psi in front
of every damping site, and then walks lambda = h' psi~ / N2 back through the adjoints of the fixed operators:
    d value = d num / N2,  num = <psi~|h'|psi~>:  the unnormalised numerator with the pattern held fixed, over the final N2.
naive=True is the mistake the tests must see: the derivative of the normalised value num / N2 with the pattern fixed,
lambda = (h' - value) psi~ / N2.

inverse=True is the kernels' reverse walk: psi in front of a site that fired is the kept one (the kernels re-walk it from the
block's snapshot), through a site that did not fire psi goes back by K0^-1 = diag(1, 1 / sqrt(1 - gamma)).  Since the last
restore that has multiplied the wire's |1> half by the product of those factors, and with it what rounding left there;
restart_above (log10 of that per-wire product) restores psi from the kept state in front of a site that would take a wire's
product past it, and clears every wire's product, as a fired site does.  RESTART_ABOVE is the library's rule: None, the kernels
have no such restart (DESIGN.md 7p has the table behind RESTART_TABLED and why it is not in the kernels).  The products and the
decisions taken from them are bookkeeping in float64 in the order of the walk, whatever the dtype.

dtype: tests/noise_oracle.py real_of.  The model around the circuit is oracle.hea_oracle's through the engines of
tests/noisy_traj_grad_reference.py.
"""
import numpy as np

from oracle import hea_oracle as O
from tests import device_traj_reference as DT
from tests import noise_oracle as NO
from tests import noisy_traj_grad_reference as NTG

ENC, ROT, CTL, TGT = DT.ENC, DT.ROT, DT.CTL, DT.TGT
RESTART_ABOVE = None                       # the library's reverse walks: K0^-1 through every site that did not fire
# the largest power of ten (as log10) at which the restarted fp64 inverse walk keeps budget(row) <= 2^-10 max|row| on every jump
# case of tests/traj_precision_cases.py, the one past 12 included (at 10^9 that one is off by 1e+4 on entries of 61)
RESTART_TABLED = 8.0


def walk(n, cfgs, x, w, nz, trajectories, seed, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', row0=0, forced=None,
         naive=False, grad=True, dtype=np.complex128, inverse=False, restart_above=None):
    """
    Per (row, trajectory), M = B * T of them in row-major order: dict with
      value [M] (no bias), num [M], N2 [M] (of the final, rescaled state), gx [M, E], gw [M, blk, 3, n] (grad=True),
      pattern  the list of fire masks [M] of the damping sites with gamma > 0 in circuit order, then the rescale masks,
      sites    per damping site with gamma > 0: (block, segment, kind, wire, slot or -1), in the same order,
      polarity per such site the mask [M]: the Pauli frame of the site's segment had an X on the wire when it was reached,
      rescaled [M] how many rescales fired, counts as replay_values,
      margin   (forced=None) the smallest relative distance of a decision from its threshold, over all (row, trajectory):
               'jump' |u N2 - gamma M| / max(u N2, gamma M), 'rescale' |N2 - 2^-200| / max(N2, 2^-200),
      level [M] the largest log10 of a wire's product of 1 / sqrt(1 - gamma) over the sites since the last fired one that the
               reverse walk meets (from the pattern alone: what inverse=True multiplies psi's rounding by without a restart),
      restarts [M] (inverse=True) how many times restart_above restored psi.
    """
    real = NO.real_of(dtype)
    x = np.asarray(x, real)
    w = np.asarray(w, real)
    B, T = x.shape[0], int(trajectories)
    words = NO.stream(B, T, row0, seed)
    jp = DT.jump_pairs(n, nz, real)
    jp64 = DT.jump_pairs(n, nz)
    M = B * T
    psi = np.zeros((M, 1 << n), dtype=dtype)
    psi[:, 0] = 1.0
    ops, pattern, rescales, sites, polarity = [], [], [], [], []
    margin = {'jump': np.inf, 'rescale': np.inf}
    fired = {'pauli': 0, 'dephasing': 0, 'jump': 0}
    nforced = [0]
    frame = np.zeros(M, dtype=np.int64)                                  # X bits of the segment's Pauli frame (for `polarity` only)
    where = [0, 0]                                                       # block, segment

    def insert(q, p, sel):
        if np.any(sel):
            NO._pauli(psi, n, q, p, sel)
            ops.append(('p', q, p, sel))
            if p in (1, 2):
                frame[sel] ^= 1 << q

    def pauli1(q, wd, p):
        err = wd[0] < np.uint64(NO.threshold(p))
        idx = ((wd[1] * np.uint64(3)) >> np.uint64(32)).astype(np.int64)
        fired['pauli'] += int(err.sum())
        for c in (1, 2, 3):
            insert(q, c, err & (idx == c - 1))

    def relax(q, site, wd, slot=-1):
        gamma = jp[site, q, 0]
        zsel = wd[2] < np.uint64(NO.threshold(jp64[site, q, 1]))
        fired['dephasing'] += int(zsel.sum())
        insert(q, 3, zsel)
        if gamma == 0.0:
            return
        i0, i1 = O._pairs(n, q)
        N2 = np.sum(psi.real ** 2 + psi.imag ** 2, axis=1)
        Mq = np.sum(psi[:, i1].real ** 2 + psi[:, i1].imag ** 2, axis=1)
        if forced is None:
            u = ((wd[3].astype(np.float64) + 0.5) * 2.0 ** -32).astype(real)
            fire = u * N2 < gamma * Mq
            margin['jump'] = min(margin['jump'], float((np.abs(u * N2 - gamma * Mq) / np.maximum(u * N2, gamma * Mq)).min()))
        else:
            fire = forced[nforced[0]]
            nforced[0] += 1
        fired['jump'] += int(fire.sum())
        pattern.append(fire)
        sites.append((where[0], where[1], site, q, slot))
        polarity.append(((frame >> q) & 1) == 1)
        ops.append(('d', q, gamma, fire, psi.copy(), 1.0 / np.sqrt(1.0 - jp64[site, q, 0])))
        f = fire[:, None]
        a0, a1 = psi[:, i0].copy(), psi[:, i1].copy()
        psi[:, i0] = np.where(f, a1, a0)
        psi[:, i1] = np.where(f, 0.0, np.sqrt(1.0 - gamma) * a1)

    def end_segment():
        if forced is None:
            N2 = np.sum(psi.real ** 2 + psi.imag ** 2, axis=1)
            small = N2 < 2.0 ** -200
            margin['rescale'] = min(margin['rescale'], float((np.abs(N2 - 2.0 ** -200) / np.maximum(N2, 2.0 ** -200)).min()))
        else:
            small = forced[len(forced) - nseg + where[1]]
        rescales.append(small)
        if np.any(small):
            psi[small] *= 2.0 ** 100
            ops.append(('s', small))
        frame[:] = 0
        where[1] += 1

    nseg = sum(1 + ld for _, ld in cfgs)
    X = np.repeat(x, T, axis=0)
    call, col, s = 0, 0, 0
    for n_enc, ld in cfgs:
        assert n_enc == n
        for q in range(n):
            NO._rx(psi, n, q, X[:, col + q])
            ops.append(('x', q, col + q))
            wd = words(call + q)
            pauli1(q, wd, nz['p1'][q])
            relax(q, ENC, wd)
        end_segment()
        col += n
        call += n
        for _ in range(ld):
            for q in range(n):
                O._ry(psi, n, q, w[s, 0, q])
                ops.append(('y', q, (s, 0, q)))
                O._rz(psi, n, q, w[s, 1, q])
                ops.append(('z', q, (s, 1, q)))
                O._ry(psi, n, q, w[s, 2, q])
                ops.append(('y', q, (s, 2, q)))
                wd = words(call + q)
                pauli1(q, wd, nz['p1'][q])
                relax(q, ROT, wd)
            call += n
            for j in range(n):
                c, t = (j + 1) % n, j
                O._cnot(psi, n, c, t)
                ops.append(('c', c, t))
                frame ^= ((frame >> c) & 1) << t
                wd = words(call + 2 * j)
                err = wd[0] < np.uint64(NO.threshold(nz['p2'][j]))
                code = ((wd[1] * np.uint64(15)) >> np.uint64(32)).astype(np.int64) + 1
                fired['pauli'] += int(err.sum())
                for p in (1, 2, 3):
                    insert(c, p, err & ((code >> 2) == p))
                    insert(t, p, err & ((code & 3) == p))
                relax(t, TGT, wd, j)
                relax(c, CTL, words(call + 2 * j + 1), j)
            call += 2 * n
            s += 1
            end_segment()
        where[0] += 1
    assert call == DT.n_calls(n, cfgs) and where[1] == nseg
    pauli = O._check_pauli(ham_pauli, ham_diag)
    NO._basis_change(psi, n, pauli)
    off, h = DT.readout_weights(n, offset, coeff, ham_diag, nz['readout01'], nz['readout10'], real)
    prob = psi.real ** 2 + psi.imag ** 2
    N2 = prob.sum(axis=1)
    num = prob @ h
    out = {'value': off + num / N2, 'num': num, 'N2': N2, 'pattern': pattern + rescales, 'sites': sites, 'polarity': polarity,
           'rescaled': sum(r.astype(np.int64) for r in rescales), 'counts': fired, 'margin': margin}
    prod = np.ones((M, n))                                               # per wire, since the last fired site
    level = np.zeros(M)
    for op in reversed(ops):
        if op[0] == 'd':
            prod[:, op[1]] *= np.where(op[3], 1.0, op[5])
            prod[op[3]] = 1.0
            level = np.maximum(level, np.log10(prod.max(axis=1)))
    out['level'] = level
    if not grad:
        return out
    hh = h[None, :] - (num / N2)[:, None] if naive else h[None, :]
    lam = psi * hh / N2[:, None]
    NTG._undo_basis_change(psi, n, pauli)
    NTG._undo_basis_change(lam, n, pauli)
    gx = np.zeros((M, x.shape[1]), dtype=real)
    gw = np.zeros((M,) + w.shape, dtype=real)
    sigma = {'x': 'X', 'y': 'Y', 'z': 'Z'}
    rot = {'x': NO._rx, 'y': O._ry, 'z': O._rz}
    prod = np.ones((M, n))                                               # inverse=True: per wire, since the last restore
    restarts = np.zeros(M, dtype=np.int64)
    limit = np.inf if restart_above is None else 10.0 ** restart_above
    for op in reversed(ops):
        if op[0] == 'p':
            NO._pauli(psi, n, op[1], op[2], op[3])
            NO._pauli(lam, n, op[1], op[2], op[3])
        elif op[0] == 'c':
            O._cnot(psi, n, op[1], op[2])
            O._cnot(lam, n, op[1], op[2])
        elif op[0] == 's':
            psi[op[1]] *= 2.0 ** -100
            lam[op[1]] *= 2.0 ** 100
        elif op[0] == 'd':
            _, q, gamma, fire, before, inv = op
            i0, i1 = O._pairs(n, q)
            f = fire[:, None]
            l0, l1 = lam[:, i0].copy(), lam[:, i1].copy()
            lam[:, i0] = np.where(f, 0.0, l0)                            # K0^dagger = K0;  L^dagger = |1><0|
            lam[:, i1] = np.where(f, l0, np.sqrt(1.0 - gamma) * l1)
            if not inverse:
                psi = before
                continue
            over = ~fire & (prod[:, q] * inv > limit)
            restore = fire | over
            restarts += over
            psi[restore] = before[restore]
            prod[restore] = 1.0
            keep = ~restore
            prod[keep, q] *= inv
            psi[np.ix_(keep, i1)] *= 1.0 / np.sqrt(1.0 - gamma)          # K0^-1
        else:
            g = O._im_inner_pauli(lam, psi, n, op[1], sigma[op[0]])
            if op[0] == 'x':
                gx[:, op[2]] = g
                ang = X[:, op[2]]
            else:
                gw[(slice(None),) + op[2]] = g
                ang = w[op[2]]
            rot[op[0]](psi, n, op[1], ang, dagger=True)
            rot[op[0]](lam, n, op[1], ang, dagger=True)
    out['gx'], out['gw'], out['restarts'] = gx, gw, restarts
    return out


def traj_grad(n, cfgs, x, w, nz, trajectories, seed, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', row0=0, naive=False,
              **kw):
    """(value[B], d value / d x [B, E], d value / d w [B, blk, 3, n]): the means over a row's T trajectories (no bias).
    kw: walk's dtype, inverse, restart_above"""
    r = walk(n, cfgs, x, w, nz, trajectories, seed, offset, coeff, ham_diag, ham_pauli, row0, naive=naive, **kw)
    B, T = np.asarray(x).shape[0], int(trajectories)
    mean = lambda a: a.reshape((B, T) + a.shape[1:]).mean(axis=1)
    return mean(r['value']), mean(r['gx']), mean(r['gw'])


def shift_grad(n, cfgs, x, w, nz, trajectories, seed, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z', row0=0,
               dtype=np.complex128):
    """
    (gx [M, E], gw [M, blk, 3, n]) per trajectory by the two-term shift rule: with the pattern held fixed num is
    a + b cos(theta) + c sin(theta) in every rotation angle, so [num(theta + pi/2) - num(theta - pi/2)] / 2 is its exact
    derivative; divided by the N2 of the unshifted walk.
    """
    real = NO.real_of(dtype)
    hp = NTG.half_pi(real)
    x = np.asarray(x, real)
    w = np.asarray(w, real)
    base = walk(n, cfgs, x, w, nz, trajectories, seed, offset, coeff, ham_diag, ham_pauli, row0, grad=False, dtype=dtype)
    num = lambda xx, ww: walk(n, cfgs, xx, ww, nz, trajectories, seed, offset, coeff, ham_diag, ham_pauli, row0,
                              forced=base['pattern'], grad=False, dtype=dtype)['num']
    M = base['N2'].shape[0]
    gx, gw = np.zeros((M, x.shape[1]), dtype=real), np.zeros((M,) + w.shape, dtype=real)
    for e in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, e] += hp
        xm[:, e] -= hp
        gx[:, e] = 0.5 * (num(xp, w) - num(xm, w)) / base['N2']
    for idx in np.ndindex(w.shape):
        wp, wm = w.copy(), w.copy()
        wp[idx] += hp
        wm[idx] -= hp
        gw[(slice(None),) + idx] = 0.5 * (num(x, wp) - num(x, wm)) / base['N2']
    return gx, gw


def DeviceTrajEngine(nz, trajectories, seed, row0=0, naive=False, **kw):
    """an engine for oracle.hea_oracle's loss functions (tests/noisy_traj_grad_reference.py model_loss_grad, dpred).
    kw: walk's dtype, inverse, restart_above; a wide engine goes with model_loss_grad(..., dtype=dtype)"""
    return NTG._Engine(lambda n, cfgs, x, w, off, co, hd, hp: traj_grad(n, cfgs, x, w, nz, trajectories, seed, off, co, hd, hp,
                                                                         row0, naive, **kw))


def coverage(r, n, T):
    """what a walk's record covers, per trajectory [M]: fired jumps, the most jumps in one block, and counts of jumps at a
    block's first encoding site, at the ring's last CTL site, on a register-selected wire (q >= 6) and under an X of the frame"""
    M = r['N2'].shape[0]
    jumps = np.zeros(M, dtype=np.int64)
    per_block = {}
    first_enc = last_ctl = high = polar = 0
    for fire, (blk, seg, kind, q, slot), pol in zip(r['pattern'], r['sites'], r['polarity']):
        jumps += fire
        per_block[blk] = per_block.get(blk, 0) + fire.astype(np.int64)
        if kind == ENC and q == 0:
            first_enc += int(fire.sum())
        if kind == CTL and slot == n - 1:
            last_ctl += int(fire.sum())
        if q >= 6:
            high += int(fire.sum())
        polar += int((fire & pol).sum())
    most = np.max(np.stack(list(per_block.values())), axis=0) if per_block else np.zeros(M, dtype=np.int64)
    return {'jumps': jumps, 'most_in_block': most, 'first_enc': first_enc, 'last_ctl': last_ctl, 'high_wire': high,
            'polarity': polar, 'dephasing': r['counts']['dephasing'], 'pauli': r['counts']['pauli']}
