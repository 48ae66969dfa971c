// hea_device_noise.hpp -- host side of the calibrated device noise model (qhea_device_noise, include/quanonet_hea.h) for the
// units that evaluate it (hea_density_device.hip, hea_density_device_grad.hip; the trajectory units hea_noise_device.hip and
// hea_noise_device_wide.hip): the checks of a setting, the composition of its channels into the four sites per wire, and for the
// trajectories the (gamma, pz) of every site and the fill of a unit's table of per-call thresholds.  No device code.
#pragma once
#include <cmath>
#include <cstddef>
#include "../../include/quanonet_hea.h"

namespace qhea {

constexpr int kDevMaxWires = 6;
enum Site { kEnc = 0, kRot = 1, kCtl = 2, kTgt = 3 };

struct Triple { double off, a, b; };

inline Triple depolarizing(double p) { const double k = 1.0 - 4.0 * p / 3.0; return {k, k, 0.0}; }

// zero-temperature T1 / T2 relaxation for time t; an infinite T1 or T2 does not decay
inline Triple relaxation(double t, double T1, double T2) {
    const double x1 = std::isinf(T1) ? 0.0 : t / T1, x2 = std::isinf(T2) ? 0.0 : t / T2;
    return {exp(-x2), exp(-x1), -expm1(-x1)};
}

inline Triple after(const Triple& second, const Triple& first) {
    return {second.off * first.off, second.a * first.a, second.a * first.b + second.b};
}

inline bool prob_ok(double p) { return p >= 0.0 && p <= 1.0; }

inline int device_noise_check(int n, const qhea_device_noise* dn) {
    if (!dn || !dn->p1 || !dn->p2 || !dn->readout01 || !dn->readout10 || !dn->t1 || !dn->t2) return QHEA_EINVAL;
    if (n < QHEA_MIN_QUBITS || n > QHEA_MAX_QUBITS || dn->n_wires != n) return QHEA_EINVAL;
    for (int q = 0; q < n; ++q) {
        if (!prob_ok(dn->p1[q]) || !prob_ok(dn->p2[q]) || !prob_ok(dn->readout01[q]) || !prob_ok(dn->readout10[q]))
            return QHEA_EINVAL;
        if (!(dn->t1[q] > 0.0) || !(dn->t2[q] > 0.0) || dn->t2[q] > 2.0 * dn->t1[q]) return QHEA_EINVAL;
    }
    for (double t : {dn->t_rx, dn->t_rot, dn->t_cx})
        if (!(t >= 0.0) || std::isinf(t)) return QHEA_EINVAL;
    return QHEA_OK;
}

// chan[site][q] for a checked setting (stride: wires per site in `chan`), lam2[j]
inline void device_noise_compose(int n, const qhea_device_noise* dn, double* chan, int stride, double* lam2) {
    const bool idle = dn->idle != 0;
    for (int q = 0; q < n; ++q) {
        const double T1 = dn->t1[q], T2 = dn->t2[q];
        const Triple d = depolarizing(dn->p1[q]);
        const double t_rot = dn->t_rot + (idle && q >= 1 ? (q - 1) * dn->t_cx : 0.0);
        const double t_tgt = idle ? (q == 0 ? n - 1 : n - q) * dn->t_cx : dn->t_cx;
        const Triple site[4] = {after(relaxation(dn->t_rx, T1, T2), d), after(relaxation(t_rot, T1, T2), d),
                                relaxation(dn->t_cx, T1, T2), relaxation(t_tgt, T1, T2)};
        for (int k = 0; k < 4; ++k) {
            double* c = chan + ((size_t)k * stride + q) * 3;
            c[0] = site[k].off; c[1] = site[k].a; c[2] = site[k].b;
        }
        lam2[q] = 16.0 * dn->p2[q] / 15.0;
    }
}

// ---- quantum-jump trajectories: one relaxation per site at its folded duration ------------------------------------------------

// an event happens iff its 32-bit word is < threshold(p) (p 2^32, floored)
inline unsigned long long threshold(double p) { return (unsigned long long)(p * 4294967296.0); }

// folded duration of site `site` on wire q (the table of the header)
inline double site_duration(int n, const qhea_device_noise* dn, int site, int q) {
    const bool idle = dn->idle != 0;
    switch (site) {
        case kEnc: return dn->t_rx;
        case kRot: return dn->t_rot + (idle && q >= 1 ? (q - 1) * dn->t_cx : 0.0);
        case kCtl: return dn->t_cx;
        default:   return idle ? (q == 0 ? n - 1 : n - q) * dn->t_cx : dn->t_cx;
    }
}

// (gamma, pz) of relaxation for time t: amplitude damping gamma, then Z with probability pz so that the off-diagonals end at
// exp(-t / T2) in total
inline void jump_pair(double t, double T1, double T2, double& gamma, double& pz) {
    const double x1 = std::isinf(T1) ? 0.0 : t / T1, x2 = std::isinf(T2) ? 0.0 : t / T2;
    gamma = 1.0 - exp(-x1);
    double f = gamma < 1.0 ? exp(-x2) / sqrt(1.0 - gamma) : 0.0;
    if (f > 1.0) f = 1.0;                                                // T2 = 2 T1 to rounding
    pz = 0.5 * (1.0 - f);
}

inline void jump_tables(int n, const qhea_device_noise* dn, double* jump) {
    for (int site = 0; site < 4; ++site)
        for (int q = 0; q < n; ++q)
            jump_pair(site_duration(n, dn, site, q), dn->t1[q], dn->t2[q], jump[((size_t)site * n + q) * 2],
                      jump[((size_t)site * n + q) * 2 + 1]);
}

// A trajectory unit's table (DevTable, WideDevTable: JumpTable<W> of hea_noise_jump.hpp, which differ in the wires they are
// sized for) from a checked setting: cthr[c] = (Pauli threshold, dephasing threshold) of call c of a block's
// template (ENC 0..n-1, ROT n..2n-1, slot j: 2n + 2j, + 1), gs[site][q] = (gamma, sqrt(1 - gamma)), the readout thresholds and
// rates per bit.  any: some event can fire.
template <class Table>
inline void fill_jump_table(int n, const qhea_device_noise* dn, Table& t, bool& any) {
    double flat[4 * QHEA_MAX_QUBITS * 2];                                // [4][n][2]
    jump_tables(n, dn, flat);
    auto jump = [&](int site, int q, int k) { return flat[((size_t)site * n + q) * 2 + k]; };
    any = false;
    for (int q = 0; q < n; ++q) {
        t.cthr[q][0] = threshold(dn->p1[q]);         t.cthr[q][1] = threshold(jump(kEnc, q, 1));
        t.cthr[n + q][0] = threshold(dn->p1[q]);     t.cthr[n + q][1] = threshold(jump(kRot, q, 1));
        t.cthr[2 * n + 2 * q][0] = threshold(dn->p2[q]);                 // slot q: the pair, and TGT of wire q
        t.cthr[2 * n + 2 * q][1] = threshold(jump(kTgt, q, 1));
        t.cthr[2 * n + 2 * q + 1][0] = 0;                                // ... CTL of wire (q + 1) mod n
        t.cthr[2 * n + 2 * q + 1][1] = threshold(jump(kCtl, (q + 1) % n, 1));
        for (int site = 0; site < 4; ++site) {
            t.gs[site][q][0] = jump(site, q, 0);
            t.gs[site][q][1] = sqrt(1.0 - jump(site, q, 0));
            any = any || jump(site, q, 0) > 0.0;
        }
        t.rthr[q][0] = threshold(dn->readout01[q]); t.rthr[q][1] = threshold(dn->readout10[q]);
        t.rd[q][0] = dn->readout01[q]; t.rd[q][1] = dn->readout10[q];
    }
    for (int c = 0; c < 4 * n; ++c) any = any || t.cthr[c][0] || t.cthr[c][1];
}

// C of the header: the Philox calls of the circuit, n + 3 n ld per block
inline unsigned jump_calls(int n, const int (&nb)[2], const int (&ld)[2]) {
    unsigned calls = 0;
    for (int g = 0; g < 2; ++g) calls += (unsigned)nb[g] * (unsigned)(n + 3 * n * ld[g]);
    return calls;
}

}  // namespace qhea
