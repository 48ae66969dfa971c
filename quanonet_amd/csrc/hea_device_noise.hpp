// hea_device_noise.hpp -- host side of the calibrated device noise model (qhea_device_noise, include/quanonet_hea.h) for the
// units that evaluate it (hea_density_device.hip, hea_density_device_grad.hip and their tiled siblings; the trajectory units hea_noise_device.hip and
// hea_noise_device_wide.hip): the checks of a setting and what opens a density-matrix call under one, the composition of its
// channels into the four sites per wire and their form in the kernels' tables, and for the trajectories the (gamma, pz) of every
// site and the fill of a unit's table of per-call thresholds.  No device code.
#pragma once
#include <cmath>
#include <cstddef>
#include "../../include/quanonet_hea.h"
#include "hea_noise_traj.hpp"

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

// What opens the three density-matrix calls under a device setting (the exact forward, loss_grad, train_steps), in the order the
// ABI reports it: the descriptor, the setting's QHEA_EINVAL cases, what the unit itself refuses (`refuse`, or none: the gradient
// unit's qubit limit and guard), then the shared checks of the uniform calls.
// noisy_call_check (hea_noise_traj.hpp, shared with the uniform calls and left as it is) reads the model itself and wants a
// qhea_noise to check; the device setting has to be checked against the model's n before it, so the model is read twice
// (host arithmetic on the descriptor) and the shared checks get an all-zero qhea_noise.  model_info appends to the record's
// block list, so the first reading goes into a record of its own: filling c.mi twice would double the sub-layer count,
// and with it the gate table of the workspace and what prep_model_kernel reads of `params`.
// (The quantum-jump entry body, jump_forward of hea_noise_jump.hpp, opens in another order -- the sampling record is refused
// between the setting and the shared checks, which get its value count, not zeros -- and keeps its own text.)
inline int device_call_check(const NoisyKind& k, const qhea_model_desc* desc, const double* ham_diag, const qhea_device_noise* dn,
                             int (*refuse)(const ModelInfo&, const qhea_device_noise*), int64_t count, const double* trunk,
                             std::initializer_list<const void*> required, void* workspace, void* stream, NoisyCall& c) {
    ModelInfo probe;
    int rc = model_info(desc, probe);
    if (rc != QHEA_OK) return rc;
    rc = device_noise_check(probe.n, dn);
    if (rc != QHEA_OK) return rc;
    if (refuse && (rc = refuse(probe, dn)) != QHEA_OK) return rc;
    const qhea_noise none{};
    return noisy_call_check(k, desc, ham_diag, &none, 0, count, trunk, required, workspace, stream, c);
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

// The forms the density-matrix kernels multiply with.  A triple's element form (off, k00, k01, k10, k11): rho00' = k00 rho00 +
// k01 rho11, rho11' = k10 rho00 + k11 rho11, the off-diagonal elements times off.  The host forms the four k: arithmetic on
// launch constants would be fp64 vector work whose results the compiler keeps in vector registers across the whole circuit loop.
inline void element_form(const Triple& t, double* c) {
    c[0] = t.off;
    c[1] = 0.5 * (1.0 + t.a + t.b); c[2] = 0.5 * (1.0 - t.a + t.b);
    c[3] = 0.5 * (1.0 - t.a - t.b); c[4] = 0.5 * (1.0 + t.a - t.b);
}
// ... and the two-qubit channel of a slot with lam = 16 p2 / 15: (keep, mix) = (1 - lam, lam / 4)
inline void slot_form(double lam, double& keep, double& mix) { keep = 1.0 - lam; mix = 0.25 * lam; }

// A checked setting's sites and slots for up to kDevMaxWires wires
struct DevSites {
    double chan[4][kDevMaxWires][3] = {}, lam2[kDevMaxWires] = {};
    DevSites(int n, const qhea_device_noise* dn) { device_noise_compose(n, dn, &chan[0][0][0], kDevMaxWires, lam2); }
    Triple at(int site, int q) const { return {chan[site][q][0], chan[site][q][1], chan[site][q][2]}; }
};

// ---- quantum-jump trajectories: one relaxation per site at its folded duration ------------------------------------------------

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
