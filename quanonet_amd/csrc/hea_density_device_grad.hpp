// hea_density_device_grad.hpp -- what the two exact gradient units under the calibrated device noise model share
// (hea_density_device_grad.hip: n <= 6, rho and O in LDS; hea_density_device_wide_grad.hip: n = 7, 8, 9 on tiles): the layout of
// one wire's record in the constants table, the scalar reads of a site's constants behind a zero the compiler cannot see
// through, a site in reverse (inverse on rho, adjoint on O), the encoding in reverse, and on the host the amplification
// log10 A_dev of a setting with the guard's bound.  hea_density_device_grad.hip explains the table and the forms.
#pragma once
#include <vector>

#include "hea_density_grad.hpp"
#include "hea_device_noise.hpp"

namespace qhea {
namespace {

// table of one wire q (doubles): [site][form][off, k00, k01, k10, k11], then the slot q's D2 and the wire's readout
constexpr int kFormFwd = 0, kFormInv = 1, kFormAdj = 2;
constexpr int kTabSite = 15, kTabSlot = 60 /* keep2, mix2, inverse keep2, inverse mix2 */, kTabRead = 64 /* r01, r10 */;
constexpr int kTabWire = 66, kTabDoubles = kTabWire * kDevMaxWires;

// A scalar zero the compiler cannot see through: a table address formed behind it belongs to the pass that forms it, so the
// loads of a pass' constants are neither hoisted ahead of the loop over the sub-layers nor shared between passes.
__device__ __forceinline__ int opaque_szero() {
    int z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    return z;
}

// one table entry in scalar registers (the address is the same in every lane)
__device__ __forceinline__ double uniform_load(const double* p) {
    const double v = *p;
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// the 2 x 2 blocks of one wire under the five constants at c: (off, k00, k01, k10, k11)
template <int S>
__device__ __forceinline__ void channel5(double2 (&e)[16], const double* c) {
    const double off = uniform_load(c), k00 = uniform_load(c + 1), k01 = uniform_load(c + 2), k10 = uniform_load(c + 3),
                 k11 = uniform_load(c + 4);
    phase_covariant<S>(e, off, k00, k01, k10, k11);
}

__device__ __forceinline__ const double* site_at(const double* tab, int q, int site, int form) {
    return tab + q * kTabWire + site * kTabSite + form * 5;
}


// site `site` of wire q in reverse: its inverse on rho, its adjoint on O
template <int S>
__device__ __forceinline__ void undo_site(double2 (&e)[16], double2 (&o)[16], const double* tab, int q, int site) {
    channel5<S>(e, site_at(tab, q, site, kFormInv));
    channel5<S>(o, site_at(tab, q, site, kFormAdj));
}

// encoding of wire q: its site, trace (slot 3 of the wire's four), RX^dagger
template <int S>
__device__ __forceinline__ void dev_undo_encoding(double2 (&e)[16], double2 (&o)[16], const double* tab, int q, double2 c,
                                                  double* tr) {
    undo_site<S>(e, o, tab, q, kEnc);
    tr[3] = pinned(trace16<S, 0>(o, e));
    unrotate_x<S>(e, c.x, c.y);
    unrotate_x<S>(o, c.x, c.y);
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// log10 A_dev of a checked setting: - sum log10 min(off, a) over the one-wire sites the circuit applies (ENC once per block,
// ROT / CTL / TGT once per sub-layer) - sum log10 (1 - lam_j) over its CNOT slots; +inf for a singular channel
// `layer`: of the largest single unit instead -- one sub-layer's sites and slots, with the ENC sites if the circuit encodes at
// all (every block does, so some first sub-layer carries them); the ENC sites alone for a circuit without sub-layers
double device_log10_amplification(const ModelInfo& mi, const qhea_device_noise* dn, bool layer = false) {
    const int n = mi.n;
    for (int q = 0; q < n; ++q)
        if (!(dn->p1[q] < 0.75) || !(dn->p2[q] < 15.0 / 16.0)) return INFINITY;
    std::vector<double> chan((size_t)4 * n * 3), lam2((size_t)n);
    device_noise_compose(n, dn, chan.data(), n, lam2.data());
    const double enc = (double)(mi.sh.E / n), sub = (double)mi.sh.blk;
    const double slots = layer && sub > 1.0 ? 1.0 : sub;
    const double count[4] = {layer && enc > 1.0 ? 1.0 : enc, slots, slots, slots};
    double sum = 0.0;
    for (int k = 0; k < 4; ++k) {
        if (count[k] == 0.0) continue;
        for (int q = 0; q < n; ++q) {
            const double* c = chan.data() + ((size_t)k * n + q) * 3;
            const double m = c[0] < c[1] ? c[0] : c[1];
            if (!(m > 0.0)) return INFINITY;
            sum -= count[k] * log10(m);
        }
    }
    for (int j = 0; j < n && mi.sh.blk > 0; ++j) sum -= slots * log10(1.0 - lam2[j]);
    return sum;
}

// The guard's bound on log10 A_dev.  The uniform walk's 12 (kMaxLog10Amplification) does not carry over: a site with b != 0 is
// not self-adjoint, O no longer shrinks by the factor rho grows by, and the numpy probe of tests/test_device_noise_training_abi.py
// (inverse walk against a walk over stored forward states; n = 5 with 60 and 120 sub-layers, n = 6 with 20) shows at most
// 2.1e-15 at log10 A_dev = 4, 1.3e-14 at 5, 4.5e-14 at 6, 2.4e-13 at 7, but 1.5e-12 at 8 and 1.1e-9 at 11.99.  7 is the
// largest probed value that stays under the 1e-12 the uniform bound was held to.
constexpr double kMaxLog10AmplificationDevice = 7.0;

}  // namespace
}  // namespace qhea
