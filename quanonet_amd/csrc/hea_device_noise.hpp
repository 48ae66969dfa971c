// hea_device_noise.hpp -- host side of the calibrated device noise model (qhea_device_noise, include/quanonet_hea.h) for the
// units that evaluate it (hea_density_device.hip, hea_density_device_grad.hip): the checks of a setting and the composition of
// its channels into the four sites per wire.  No device code.
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

}  // namespace qhea
