// hea_density.hpp -- what the density-matrix kernels share: the exact noisy forward (hea_density.hip) and its adjoint gradient
// (hea_density_grad.hip), and their counterparts under a device noise model (hea_density_device.hip,
// hea_density_device_grad.hip).  Element layout, bank fold, the pass over two wires, the gates and the depolarizing channels in their
// closed forms, and the forward sweep's passes; hea_density.hip describes the layout.  Host side: the dispatch on the qubit count,
// the forward launcher and the fill of what every argument record holds of the circuit.  Everything sits in an unnamed namespace:
// each translation unit compiles its own copy into its own kernels.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "hea_noise_traj.hpp"

namespace qhea {
namespace {

constexpr int kDensThreads = 256;
constexpr int kDensStateBytes = 4096 * (int)sizeof(double2);             // 256 threads x 16 elements

struct DensArgs {
    const double4* gates;                   // prep table, entry 0 = padding entry -n
    const double2* cs;                      // [B, E]
    const double* diag;                     // ham_diag or NULL
    const double* bias;                     // model bias or NULL
    double off, co, q;                      // H = off + co sum P_i; readout flip probability
    double d1_off, d1_keep, d1_mix;         // one-qubit channel: 1 - 4p/3, 1 - 2p/3, 2p/3
    double d2_keep, d2_mix;                 // two-qubit channel: 1 - lam, lam / 4 (lam = 16 p / 15)
    long B;
    int E, pauli;
    int nb[2], ld[2];
    double* pred;
    double* sd;                             // or NULL
};

struct Cx { double re, im; };
struct U2 { Cx u00, u01, u10, u11; };

__device__ __forceinline__ double2 cmul(Cx a, double2 b) { return make_double2(a.re * b.x - a.im * b.y, a.re * b.y + a.im * b.x); }
__device__ __forceinline__ double2 cmulc(Cx a, double2 b) { return make_double2(a.re * b.x + a.im * b.y, a.re * b.y - a.im * b.x); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }

// the 2 x 2 blocks of one wire (local elements base + S {0: rho00, 1: rho10, 2: rho01, 3: rho11}): rho <- U rho U^dagger
template <int S>
__device__ __forceinline__ void apply_gate(double2 (&e)[16], const U2& u) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int b = S == 1 ? 4 * m : m;
        double2 r[4];
#pragma unroll
        for (int c = 0; c < 2; ++c) {                                    // U on the row index
            const double2 x0 = e[b + S * (2 * c)], x1 = e[b + S * (2 * c + 1)];
            r[2 * c] = cadd(cmul(u.u00, x0), cmul(u.u01, x1));
            r[2 * c + 1] = cadd(cmul(u.u10, x0), cmul(u.u11, x1));
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {                                    // U* on the column index
            const double2 x0 = r[a], x1 = r[a + 2];
            e[b + S * a] = cadd(cmulc(u.u00, x0), cmulc(u.u01, x1));
            e[b + S * (a + 2)] = cadd(cmulc(u.u10, x0), cmulc(u.u11, x1));
        }
    }
}

// the encoding gate RX(x) of a wire from (cos, sin)(x / 2)
__device__ __forceinline__ U2 encoding_rx(double2 c) { return U2{{c.x, 0.0}, {0.0, -c.y}, {0.0, -c.y}, {c.x, 0.0}}; }

// one-qubit depolarizing channel on the same blocks
template <int S>
__device__ __forceinline__ void depolarize1(double2 (&e)[16], const DensArgs& a) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int b = S == 1 ? 4 * m : m;
        const double2 d0 = e[b], d1 = e[b + 3 * S];
        e[b] = make_double2(a.d1_keep * d0.x + a.d1_mix * d1.x, a.d1_keep * d0.y + a.d1_mix * d1.y);
        e[b + 3 * S] = make_double2(a.d1_keep * d1.x + a.d1_mix * d0.x, a.d1_keep * d1.y + a.d1_mix * d0.y);
        e[b + S].x *= a.d1_off; e[b + S].y *= a.d1_off;
        e[b + 2 * S].x *= a.d1_off; e[b + 2 * S].y *= a.d1_off;
    }
}

// a phase-covariant one-wire channel in its element form (element_form of hea_device_noise.hpp) on the same blocks:
// rho00' = k00 rho00 + k01 rho11, rho11' = k10 rho00 + k11 rho11, the off-diagonal elements times off.  The device units fetch
// the five constants their own way.  depolarize1 above is the case k00 = k11, k01 = k10 but keeps its text: written through
// this body, the uniform kernels' code changes (profiles/r28_device_code_identity.txt).
template <int S>
__device__ __forceinline__ void phase_covariant(double2 (&e)[16], double off, double k00, double k01, double k10, double k11) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int b = S == 1 ? 4 * m : m;
        const double2 d0 = e[b], d1 = e[b + 3 * S];
        e[b] = make_double2(k00 * d0.x + k01 * d1.x, k00 * d0.y + k01 * d1.y);
        e[b + 3 * S] = make_double2(k10 * d0.x + k11 * d1.x, k10 * d0.y + k11 * d1.y);
        e[b + S].x *= off; e[b + S].y *= off;
        e[b + 2 * S].x *= off; e[b + 2 * S].y *= off;
    }
}

// wire q's pending gates of sub-layer s: (encoding RX, channel), fused RY RZ RY, channel
template <int N, int S>
__device__ __forceinline__ void wire_gates(double2 (&e)[16], const DensArgs& a, const double2* csr, int s, int col, bool enc,
                                           int q) {
    if (enc) {
        const double2 c = csr[col + q];
        apply_gate<S>(e, encoding_rx(c));
        depolarize1<S>(e, a);
    }
    const double4 v = a.gates[2 * (s * N + q + N)];                      // (u00, u01); u10 = -conj(u01), u11 = conj(u00)
    apply_gate<S>(e, U2{{v.x, v.y}, {v.z, v.w}, {-v.z, v.w}, {v.x, -v.y}});
    depolarize1<S>(e, a);
}

// CNOT(c -> t) on both indices (local bits: 0 / 1 = t's row / column bit, 2 / 3 = c's), then the two-qubit channel
// (keep, mix) = (1 - lam, lam / 4): the uniform one, or a slot's own under a device noise model
__device__ __forceinline__ void cnot_depolarize2(double2 (&e)[16], double keep, double mix) {
    double2 r[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) r[k] = e[k ^ ((k >> 2) & 1) ^ (((k >> 3) & 1) << 1)];
    const double sx = (r[0].x + r[3].x) + (r[12].x + r[15].x), sy = (r[0].y + r[3].y) + (r[12].y + r[15].y);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool eq = k == 0 || k == 3 || k == 12 || k == 15;          // row bits (c, t) = column bits
        e[k].x = eq ? keep * r[k].x + mix * sx : keep * r[k].x;
        e[k].y = eq ? keep * r[k].y + mix * sy : keep * r[k].y;
    }
}

// LDS slot of element i of a row: the low nibble folded with the higher ones (fold is linear, so a pass folds its base once)
__device__ __forceinline__ int fold(int i) { return ((i >> 4) ^ (i >> 8)) & 15; }
template <int N> __device__ __forceinline__ int slot_fold(int slot) {
    return N == 2 ? slot & 15 : N == 3 ? (slot & 3) * 5 : 0;             // rows that share a 16-lane group
}

// the pass over wires (t, c) = (J, J + 1 mod N): thread `rank` of the row owns the elements base | kt << 2t | kc << 2c
template <int N, int J> struct Pass {
    static constexpr int t = J, c = (J + 1) % N, lo = t < c ? t : c, hi = t < c ? c : t;
    __device__ static __forceinline__ int base(int rank) {
        int r = rank;
        r = ((r >> (2 * lo)) << (2 * lo + 2)) | (r & ((1 << (2 * lo)) - 1));
        r = ((r >> (2 * hi)) << (2 * hi + 2)) | (r & ((1 << (2 * hi)) - 1));
        return r;
    }
    static constexpr int local(int k) { return ((k & 3) << (2 * t)) | ((k >> 2) << (2 * c)); }
    __device__ static __forceinline__ void load(double2 (&e)[16], const double2* row, int b) {
#pragma unroll
        for (int k = 0; k < 16; ++k) e[k] = row[b ^ (local(k) ^ fold(local(k)))];
    }
    __device__ static __forceinline__ void store(const double2 (&e)[16], double2* row, int b) {
#pragma unroll
        for (int k = 0; k < 16; ++k) row[b ^ (local(k) ^ fold(local(k)))] = e[k];
    }
};

template <int N, int J>
__device__ __forceinline__ void ring_passes(double2* row, int rank, int sf, const DensArgs& a, const double2* csr, int s,
                                            int col, bool enc, bool first) {
    if constexpr (J < N) {
        using P = Pass<N, J>;
        const int i0 = P::base(rank), b = i0 ^ fold(i0) ^ sf;
        double2 e[16];
        if (J == 0 && first) {                                           // rho = |0><0|
#pragma unroll
            for (int k = 0; k < 16; ++k) e[k] = make_double2(k == 0 && rank == 0 ? 1.0 : 0.0, 0.0);
        } else {
            P::load(e, row, b);
        }
        if (J == 0) wire_gates<N, 1>(e, a, csr, s, col, enc, P::t);
        if (J <= N - 2) wire_gates<N, 4>(e, a, csr, s, col, enc, P::c);
        cnot_depolarize2(e, a.d2_keep, a.d2_mix);
        P::store(e, row, b);
        __syncthreads();
        ring_passes<N, J + 1>(row, rank, sf, a, csr, s, col, enc, false);
    }
}

// one-qubit gates on every wire, two wires per pass (J even; the last pass of an odd N wraps to wire 0 and leaves it alone):
// KIND 0 = a block's encoding RX with its channel (blocks without sub-layers), 1 = H, 2 = H S^dagger (read-out basis, no noise)
template <int N, int J, int KIND>
__device__ __forceinline__ void wire_passes(double2* row, int rank, int sf, const DensArgs& a, const double2* csr, int col,
                                            bool first) {
    if constexpr (J < N) {
        using P = Pass<N, J>;
        const int i0 = P::base(rank), b = i0 ^ fold(i0) ^ sf;
        double2 e[16];
        if (J == 0 && first) {
#pragma unroll
            for (int k = 0; k < 16; ++k) e[k] = make_double2(k == 0 && rank == 0 ? 1.0 : 0.0, 0.0);
        } else {
            P::load(e, row, b);
        }
        const U2 h = KIND == 1 ? U2{{M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {-M_SQRT1_2, 0.0}}
                               : U2{{M_SQRT1_2, 0.0}, {0.0, -M_SQRT1_2}, {M_SQRT1_2, 0.0}, {0.0, M_SQRT1_2}};
        if (KIND == 0) {
            const double2 c0 = csr[col + P::t];
            apply_gate<1>(e, encoding_rx(c0));
            depolarize1<1>(e, a);
            if (J + 1 < N) {
                const double2 c1 = csr[col + P::c];
                apply_gate<4>(e, encoding_rx(c1));
                depolarize1<4>(e, a);
            }
        } else {
            apply_gate<1>(e, h);
            if (J + 1 < N) apply_gate<4>(e, h);
        }
        P::store(e, row, b);
        __syncthreads();
        wire_passes<N, J + 2, KIND>(row, rank, sf, a, csr, col, false);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// The family's kernels exist for n = 2..6 (4^n elements per row in LDS): f(std::integral_constant<int, n>) for the call's n
template <class F>
int dispatch_n(int n, F&& f) {
    switch (n) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        default: return QHEA_EUNSUPPORTED;
    }
}

// a forward kernel (density_fwd_kernel<N>, density_dev_fwd_kernel<N>): 256 / 4^(n-2) rows per workgroup; the state, h'[D], h2'[D]
template <int N, class Args>
int launch_density_fwd(void (*kernel)(Args), const Args& a, hipStream_t st) {
    constexpr int RPW = kDensThreads / (1 << (2 * N - 4));
    constexpr size_t smem = kDensStateBytes + 2 * (1 << N) * sizeof(double);
    return launch_dynamic_lds(kernel, dim3((unsigned)((a.B + RPW - 1) / RPW)), dim3(kDensThreads), smem, st, a);
}

struct DensLayout { size_t off_gates, off_cs, total; };

DensLayout dens_layout(const ModelInfo& mi, int64_t B) {
    const TableLayout t = table_layout(mi, B);
    return DensLayout{t.off_gates, t.off_cs, t.end};
}

// what every argument record of the family holds of the circuit, its read-out and the prep tables (DensArgs, and the device
// units' DensDevArgs and DevGradArgs, which name these members alike)
template <class Args>
void circuit_args(Args& a, const qhea_model_desc* desc, const ModelInfo& mi, const double* params, const double* ham_diag,
                  int64_t batch, const double4* gates, const double2* cs) {
    a.gates = gates; a.cs = cs; a.diag = ham_diag;
    a.bias = mi.has_bias ? params + mi.off_bias : nullptr;
    a.off = desc->ham_offset; a.co = desc->ham_coeff;
    a.B = batch; a.E = (int)mi.sh.E; a.pauli = desc->ham_pauli;
    for (int g = 0; g < 2; ++g) { a.nb[g] = mi.nb[g]; a.ld[g] = mi.ld[g]; }
}

// everything of DensArgs but the outputs (pred, sd)
DensArgs dens_args(const qhea_model_desc* desc, const ModelInfo& mi, const qhea_noise* noise, const double* params,
                   const double* ham_diag, int64_t batch, const double4* gates, const double2* cs) {
    DensArgs a{};
    circuit_args(a, desc, mi, params, ham_diag, batch, gates, cs);
    a.q = noise->readout;
    a.d1_off = 1.0 - 4.0 * noise->p1 / 3.0; a.d1_keep = 1.0 - 2.0 * noise->p1 / 3.0; a.d1_mix = 2.0 * noise->p1 / 3.0;
    const double lam = 16.0 * noise->p2 / 15.0;
    a.d2_keep = 1.0 - lam; a.d2_mix = lam / 4.0;
    return a;
}
}  // namespace
}  // namespace qhea
