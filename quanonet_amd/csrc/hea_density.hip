// hea_density.hip -- qhea_model_forward_noisy_exact: the model forward under the noise model of qhea_model_forward_noisy
// (include/quanonet_hea.h), computed exactly by carrying the density matrix rho through the circuit: per row the expectation of
// a read value and the standard deviation of one shot.  tests/density_reference.py restates it in numpy.
//
// Layout: vec(rho) of n qubits is a state of 2n index bits; bit 2q is wire q's row bit, bit 2q + 1 its column bit, so a gate on
// wire q touches two adjacent index bits and a CNOT with its channel four.  A row's 4^n elements live in LDS (16 bytes each); a
// thread owns 16 of them per pass: the elements that differ in the row and column bits of two wires.  4^(n-2) threads serve a
// row, a workgroup of 256 threads holds 256 / 4^(n-2) rows (256, 64, 16, 4, 1 for n = 2..6): always 64 KiB of state.
// A sub-layer is n passes; pass j loads wires (t, c) = (j, j + 1 mod n), applies the one-qubit gates still pending on them
// (the fused RY RZ RY, preceded by the encoding RX in a block's first sub-layer; wires 0 and 1 in pass 0, wire j + 1 in passes
// 1..n-2, none in the last) each with its depolarizing channel, then CNOT(c -> t) as a renaming of the 16 registers and the
// two-qubit channel, and stores.  One barrier per pass.  The low four bits of an element's LDS slot are XORed with the higher
// nibbles of its index (and with the row slot where several rows share a lane group), which spreads every pass' reads over the
// 16-byte bank quads.
//
// Read-out: H (X) or H S^dagger (Y) on every wire as one-qubit passes without noise; p = diag rho.  The readout confusion is
// symmetric, so it is applied to the value table instead of p: a workgroup mixes h[k] and h[k]^2 over the n bits once, before
// the circuit, and one thread per row adds p_k h'[k] and p_k h2'[k] in index order.  Nothing depends on the batch, the grid or
// other rows, and there are no atomics: a row's result is bitwise the same in any call.
#include <cmath>
#include <cstdint>

#include "hea_noise.hpp"

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

// wire q's pending gates of sub-layer s: (encoding RX, channel), fused RY RZ RY, channel
template <int N, int S>
__device__ __forceinline__ void wire_gates(double2 (&e)[16], const DensArgs& a, const double2* csr, int s, int col, bool enc,
                                           int q) {
    if (enc) {
        const double2 c = csr[col + q];
        apply_gate<S>(e, U2{{c.x, 0.0}, {0.0, -c.y}, {0.0, -c.y}, {c.x, 0.0}});
        depolarize1<S>(e, a);
    }
    const double4 v = a.gates[2 * (s * N + q + N)];                      // (u00, u01); u10 = -conj(u01), u11 = conj(u00)
    apply_gate<S>(e, U2{{v.x, v.y}, {v.z, v.w}, {-v.z, v.w}, {v.x, -v.y}});
    depolarize1<S>(e, a);
}

// CNOT(c -> t) on both indices (local bits: 0 / 1 = t's row / column bit, 2 / 3 = c's), then the two-qubit channel
__device__ __forceinline__ void cnot_depolarize2(double2 (&e)[16], const DensArgs& a) {
    double2 r[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) r[k] = e[k ^ ((k >> 2) & 1) ^ (((k >> 3) & 1) << 1)];
    const double sx = (r[0].x + r[3].x) + (r[12].x + r[15].x), sy = (r[0].y + r[3].y) + (r[12].y + r[15].y);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool eq = k == 0 || k == 3 || k == 12 || k == 15;          // row bits (c, t) = column bits
        e[k].x = eq ? a.d2_keep * r[k].x + a.d2_mix * sx : a.d2_keep * r[k].x;
        e[k].y = eq ? a.d2_keep * r[k].y + a.d2_mix * sy : a.d2_keep * r[k].y;
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
        cnot_depolarize2(e, a);
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
            apply_gate<1>(e, U2{{c0.x, 0.0}, {0.0, -c0.y}, {0.0, -c0.y}, {c0.x, 0.0}});
            depolarize1<1>(e, a);
            if (J + 1 < N) {
                const double2 c1 = csr[col + P::c];
                apply_gate<4>(e, U2{{c1.x, 0.0}, {0.0, -c1.y}, {0.0, -c1.y}, {c1.x, 0.0}});
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

template <int N>
__global__ __launch_bounds__(kDensThreads) void density_fwd_kernel(DensArgs a) {
    constexpr int TPR = 1 << (2 * N - 4), RPW = kDensThreads / TPR, D = 1 << N, NE = 1 << (2 * N);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];      // state, then h'[D], h2'[D]
    double2* state = reinterpret_cast<double2*>(dens_lds);
    double* hv = reinterpret_cast<double*>(dens_lds + kDensStateBytes);
    const int tid = threadIdx.x, slot = tid / TPR, rank = tid % TPR;
    long r = (long)blockIdx.x * RPW + slot;
    const bool live = r < a.B;
    if (!live) r = a.B - 1;                                              // a tail slot repeats the last row and stores nothing
    const double2* csr = a.cs + r * a.E;
    double2* row = state + slot * NE;
    const int sf = slot_fold<N>(slot);

    // value tables under the readout confusion: n two-point mixes of h and h^2
    double h = 0.0, h2 = 0.0;
    if (tid < D) {
        h = a.diag ? a.diag[tid] : a.off + a.co * (double)(N - 2 * (int)__popc(tid));
        h2 = h * h;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (tid < D) { hv[tid] = h; hv[D + tid] = h2; }
        __syncthreads();
        if (tid < D) {
            h = (1.0 - a.q) * h + a.q * hv[tid ^ (1 << i)];
            h2 = (1.0 - a.q) * h2 + a.q * hv[D + (tid ^ (1 << i))];
        }
        __syncthreads();
    }
    if (tid < D) { hv[tid] = h; hv[D + tid] = h2; }

    int s = 0, col = 0;
    bool first = true;
    for (int g = 0; g < 2; ++g) {
        for (int b = 0; b < a.nb[g]; ++b) {
            if (a.ld[g] == 0) {
                wire_passes<N, 0, 0>(row, rank, sf, a, csr, col, first);
                first = false;
            }
            for (int l = 0; l < a.ld[g]; ++l, ++s) {
                ring_passes<N, 0>(row, rank, sf, a, csr, s, col, l == 0, first);
                first = false;
            }
            col += N;
        }
    }
    if (first) {                                                         // no block at all: rho = |0><0|
        for (int i = rank; i < NE; i += TPR) row[i] = make_double2(0.0, 0.0);
        __syncthreads();
        if (rank == 0) row[fold(0) ^ sf] = make_double2(1.0, 0.0);
        __syncthreads();
    }
    if (a.pauli == QHEA_PAULI_X) wire_passes<N, 0, 1>(row, rank, sf, a, csr, 0, false);
    else if (a.pauli == QHEA_PAULI_Y) wire_passes<N, 0, 2>(row, rank, sf, a, csr, 0, false);

    if (rank == 0 && live) {
        double m1 = 0.0, m2 = 0.0;
        for (int k = 0; k < D; ++k) {
            int i = 0;
#pragma unroll
            for (int w = 0; w < N; ++w) i |= ((k >> w) & 1) * (3 << (2 * w));
            const double p = row[i ^ fold(i) ^ sf].x;
            m1 += p * hv[k];
            m2 += p * hv[D + k];
        }
        a.pred[r] = m1 + (a.bias ? a.bias[0] : 0.0);
        if (a.sd) {
            const double var = m2 - m1 * m1;
            a.sd[r] = var > 0.0 ? sqrt(var) : 0.0;
        }
    }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct DensLayout { size_t off_gates, off_cs, total; };

DensLayout dens_layout(const NoiseShape& ns, int64_t B) {
    DensLayout L{};
    size_t p = 256;                                                      // header (prep_model_kernel stamps it)
    L.off_gates = p; p = align256(p + (size_t)(ns.blk + 2) * ns.n * 2 * sizeof(double4));
    L.off_cs = p;    p = align256(p + (size_t)B * ns.E * sizeof(double2));
    L.total = p;
    return L;
}

bool rates_ok(const qhea_noise* nz) {
    if (!nz) return false;
    for (double p : {nz->p1, nz->p2, nz->readout})
        if (!(p >= 0.0 && p <= 1.0)) return false;
    return true;
}

template <int N>
int launch_density(const DensArgs& a, hipStream_t st) {
    constexpr int RPW = kDensThreads / (1 << (2 * N - 4));
    constexpr size_t smem = kDensStateBytes + 2 * (1 << N) * sizeof(double);
    // every launch: the attribute is per device, and a process may drive more than one
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(density_fwd_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)smem) != hipSuccess)
        return QHEA_ELAUNCH;
    hipLaunchKernelGGL(density_fwd_kernel<N>, dim3((unsigned)((a.B + RPW - 1) / RPW)), dim3(kDensThreads), smem, st, a);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_exact_noisy_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    NoiseShape ns;
    if (batch < 0 || noise_model_shape(desc, ns) != QHEA_OK) return 0;
    return dens_layout(ns, batch).total;
}

int qhea_model_forward_noisy_exact(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                                   const double* params, const double* ham_diag, const qhea_noise* noise, double* pred,
                                   double* shot_std, void* workspace, size_t workspace_bytes, void* stream) {
    NoiseShape ns;
    int rc = noise_model_shape(desc, ns);
    if (rc != QHEA_OK) return rc;
    if (!rates_ok(noise)) return QHEA_EINVAL;
    if (ns.n > 6) return QHEA_EUNSUPPORTED;                              // 4^n elements per row in LDS
    const bool pauli_ok = desc->ham_pauli == QHEA_PAULI_Z || ((desc->ham_pauli == QHEA_PAULI_X ||
                                                               desc->ham_pauli == QHEA_PAULI_Y) && !ham_diag);
    if (!pauli_ok || batch < 0) return QHEA_EINVAL;
    if (batch == 0) return QHEA_OK;
    if (!branch || !params || !pred || (desc->model == QHEA_MODEL_QUANONET && !trunk)) return QHEA_EINVAL;
    const DensLayout L = dens_layout(ns, batch);
    if (!workspace || workspace_bytes < L.total) return QHEA_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double4* gates = reinterpret_cast<double4*>(ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(ws + L.off_cs);
    rc = launch_noise_prep(desc, batch, branch, trunk, params, gates, cs, ws, st);
    if (rc != QHEA_OK) return rc;

    DensArgs a{};
    a.gates = gates; a.cs = cs; a.diag = ham_diag;
    a.bias = ns.off_bias >= 0 ? params + ns.off_bias : nullptr;
    a.off = desc->ham_offset; a.co = desc->ham_coeff; a.q = noise->readout;
    a.d1_off = 1.0 - 4.0 * noise->p1 / 3.0; a.d1_keep = 1.0 - 2.0 * noise->p1 / 3.0; a.d1_mix = 2.0 * noise->p1 / 3.0;
    const double lam = 16.0 * noise->p2 / 15.0;
    a.d2_keep = 1.0 - lam; a.d2_mix = lam / 4.0;
    a.B = batch; a.E = ns.E; a.pauli = desc->ham_pauli;
    for (int g = 0; g < 2; ++g) { a.nb[g] = ns.nb[g]; a.ld[g] = ns.ld[g]; }
    a.pred = pred; a.sd = shot_std;
    switch (ns.n) {
        case 2: return launch_density<2>(a, st);
        case 3: return launch_density<3>(a, st);
        case 4: return launch_density<4>(a, st);
        case 5: return launch_density<5>(a, st);
        case 6: return launch_density<6>(a, st);
        default: return QHEA_EUNSUPPORTED;
    }
}

}  // extern "C"
