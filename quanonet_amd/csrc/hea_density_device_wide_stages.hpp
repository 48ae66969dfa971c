// hea_density_device_wide_stages.hpp -- the stages of the exact noisy forward at n = 7, 8, 9 under the calibrated device noise
// model: the per-stage record, the stage wire map, the ring and one-qubit stage kernels, the value-table kernel and
// launch_density_dev_wide, the launch sequence of one call.  hea_density_device_wide.hip describes them and is their entry point;
// hea_density_device_wide_grad.hip runs the same sequence as the forward sweep of the adjoint gradient, so that its pred is the
// forward's bit for bit.  Everything sits in an unnamed namespace: each unit compiles its own copy into its own kernels.
#pragma once
#include "hea_density_wide.hpp"
#include "hea_device_noise.hpp"

namespace qhea {
namespace {

constexpr int kDevWideMaxWires = 9;         // kDevMaxWires sizes the n <= 6 kernels' record and stays

struct DevStageArgs {
    const double4* gates;                   // prep table, entry 0 = padding entry -n
    const double2* cs;                      // [B, E]
    double chan[4][6][5];                   // [site][local wire] (off, k00, k01, k10, k11): the triple's element form
    double keep2[6], mix2[6];               // two-qubit channel of local pass LJ's slot: 1 - lam, lam / 4
    int E;
};

struct DevValueArgs {
    const double* diag;                     // ham_diag or NULL
    double off, co;                         // H = off + co sum P_i
    double r01[kDevWideMaxWires], r10[kDevWideMaxWires];    // P(read 1 | 0), P(read 0 | 1) per bit
};

// global wire of local wire L of a stage
template <int N, int STAGE>
constexpr int global_wire(int L) { return STAGE == 0 || L < 2 ? L : L + N - 6; }

// the phase-covariant channel of site SITE on local wire L, its constants scalars of the launch
template <int S, int SITE, int L>
__device__ __forceinline__ void stage_channel(double2 (&e)[16], const DevStageArgs& a) {
    phase_covariant<S>(e, a.chan[SITE][L][0], a.chan[SITE][L][1], a.chan[SITE][L][2], a.chan[SITE][L][3], a.chan[SITE][L][4]);
}

// local wire L's pending gates of sub-layer s: (encoding RX, its site), fused RY RZ RY, its site
template <int N, int STAGE, int S, int L>
__device__ __forceinline__ void dev_wide_wire_gates(double2 (&e)[16], const DevStageArgs& a, const double2* csr, int s, int col,
                                                    bool enc) {
    constexpr int Q = global_wire<N, STAGE>(L);
    if (enc) {
        const double2 c = csr[col + Q];
        apply_gate<S>(e, encoding_rx(c));
        stage_channel<S, kEnc, L>(e, a);
    }
    const double4 v = a.gates[2 * (s * N + Q + N)];                      // (u00, u01); u10 = -conj(u01), u11 = conj(u00)
    apply_gate<S>(e, U2{{v.x, v.y}, {v.z, v.w}, {-v.z, v.w}, {v.x, -v.y}});
    stage_channel<S, kRot, L>(e, a);
}

// ring pass J of the circuit's n wires (slot J) on the tile that holds both of its wires
template <int N, int J>
__device__ __forceinline__ void dev_wide_ring_pass(double2* lds, int rank, const DevStageArgs& a, const double2* csr, int s,
                                                   int col, bool enc) {
    constexpr int STAGE = J < 5 ? 0 : 1, LJ = J < 5 ? J : J - N + 6;
    using P = Pass<6, LJ>;
    static_assert(global_wire<N, STAGE>(P::t) == J && global_wire<N, STAGE>(P::c) == (J + 1) % N, "the pass serves slot J");
    const int i0 = P::base(rank), b = i0 ^ fold(i0);
    double2 e[16];
    P::load(e, lds, b);
    if (J == 0) dev_wide_wire_gates<N, STAGE, 1, P::t>(e, a, csr, s, col, enc);
    if (J <= N - 2) dev_wide_wire_gates<N, STAGE, 4, P::c>(e, a, csr, s, col, enc);
    cnot_depolarize2(e, a.keep2[LJ], a.mix2[LJ]);
    stage_channel<1, kTgt, P::t>(e, a);
    stage_channel<4, kCtl, P::c>(e, a);
    P::store(e, lds, b);
    __syncthreads();
}
template <int N, int J, int JEND>
__device__ __forceinline__ void dev_wide_ring_passes(double2* lds, int rank, const DevStageArgs& a, const double2* csr, int s,
                                                     int col, bool enc) {
    if constexpr (J < JEND) {
        dev_wide_ring_pass<N, J>(lds, rank, a, csr, s, col, enc);
        dev_wide_ring_passes<N, J + 1, JEND>(lds, rank, a, csr, s, col, enc);
    }
}

// a ring stage of sub-layer s: stage A passes 0..4, stage B passes 5..n-1.  Grid: rows x 4^(n-6) workgroups, tile fastest
template <int N, int STAGE>
__global__ __launch_bounds__(kDensThreads) void density_dev_wide_ring_kernel(DevStageArgs a, double2* rho, int s, int col, int enc,
                                                                             int first) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    double2* row = rho + ((size_t)r << (2 * N));
    const double2* csr = a.cs + r * a.E;
    tile_load<N, STAGE>(lds, row, tile, tid, first != 0);
    if (STAGE == 0) dev_wide_ring_passes<N, 0, 5>(lds, tid, a, csr, s, col, enc != 0);
    else dev_wide_ring_passes<N, 5, N>(lds, tid, a, csr, s, col, enc != 0);
    tile_store<N, STAGE>(lds, row, tile, tid);
}

// one-qubit gates on the local wires (LJ, LJ + 1) of a tile, those of them the stage serves: kind 0 = a block's encoding RX
// with its kEnc site (dev_enc_passes on tiles), 1 = H, 2 = H S^dagger (read-out basis, no noise)
template <int N, int STAGE, int LJ>
__device__ __forceinline__ void dev_wide_wire_pass(double2* lds, int rank, const DevStageArgs& a, const double2* csr, int col,
                                                   int kind) {
    constexpr int served = STAGE ? 12 - N : 0;                           // stage B: local wire >= 12 - n is global wire >= 6
    constexpr bool T = LJ >= served, C = LJ + 1 >= served;
    if constexpr (T || C) {
        using P = Pass<6, LJ>;
        const int i0 = P::base(rank), b = i0 ^ fold(i0);
        double2 e[16];
        P::load(e, lds, b);
        const U2 h = kind == 1 ? U2{{M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {-M_SQRT1_2, 0.0}}
                               : U2{{M_SQRT1_2, 0.0}, {0.0, -M_SQRT1_2}, {M_SQRT1_2, 0.0}, {0.0, M_SQRT1_2}};
        if (T) {
            apply_gate<1>(e, kind == 0 ? encoding_rx(csr[col + global_wire<N, STAGE>(LJ)]) : h);
            if (kind == 0) stage_channel<1, kEnc, LJ>(e, a);
        }
        if (C) {
            apply_gate<4>(e, kind == 0 ? encoding_rx(csr[col + global_wire<N, STAGE>(LJ + 1)]) : h);
            if (kind == 0) stage_channel<4, kEnc, LJ + 1>(e, a);
        }
        P::store(e, lds, b);
        __syncthreads();
    }
}

// a one-qubit stage: stage A wires 0..5, stage B wires 6..n-1; kind 3 = no gate at all (a circuit without blocks: stage A
// with `first` writes rho = |0><0|)
template <int N, int STAGE>
__global__ __launch_bounds__(kDensThreads) void density_dev_wide_wires_kernel(DevStageArgs a, double2* rho, int col, int kind,
                                                                              int first) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    double2* row = rho + ((size_t)r << (2 * N));
    const double2* csr = a.cs + r * a.E;
    tile_load<N, STAGE>(lds, row, tile, tid, first != 0);
    if (kind != 3) {
        dev_wide_wire_pass<N, STAGE, 0>(lds, tid, a, csr, col, kind);
        dev_wide_wire_pass<N, STAGE, 2>(lds, tid, a, csr, col, kind);
        dev_wide_wire_pass<N, STAGE, 4>(lds, tid, a, csr, col, kind);
    }
    tile_store<N, STAGE>(lds, row, tile, tid);
}

// value tables under the asymmetric readout confusion: per bit, h'[k] = (1 - f) h[k] + f h[k ^ bit], f = P(the bit of k is
// misread); hv = h'[2^n], then h2'[2^n].  One workgroup
template <int N>
__global__ __launch_bounds__(512) void density_dev_wide_values_kernel(DevValueArgs a, double* hv) {
    constexpr int D = 1 << N;
    __shared__ double sh[2 * 512];
    const int tid = threadIdx.x;
    double h = 0.0, h2 = 0.0;
    if (tid < D) {
        h = a.diag ? a.diag[tid] : a.off + a.co * (double)(N - 2 * (int)__popc(tid));
        h2 = h * h;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (tid < D) { sh[tid] = h; sh[D + tid] = h2; }
        __syncthreads();
        if (tid < D) {
            const double f = (tid >> i) & 1 ? a.r10[i] : a.r01[i];
            h = (1.0 - f) * h + f * sh[tid ^ (1 << i)];
            h2 = (1.0 - f) * h2 + f * sh[D + (tid ^ (1 << i))];
        }
        __syncthreads();
    }
    if (tid < D) { hv[tid] = h; hv[D + tid] = h2; }
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// A checked setting's sites and slots for up to kDevWideMaxWires wires (DevSites of hea_device_noise.hpp is sized for six)
struct WideDevSites {
    double chan[4][kDevWideMaxWires][3] = {}, lam2[kDevWideMaxWires] = {};
    WideDevSites(int n, const qhea_device_noise* dn) { device_noise_compose(n, dn, &chan[0][0][0], kDevWideMaxWires, lam2); }
    Triple at(int site, int q) const { return {chan[site][q][0], chan[site][q][1], chan[site][q][2]}; }
};

// the record of a stage: local wire l is global wire l (stage A), or l < 2 ? l : l + n - 6 (stage B); local pass LJ is slot
// LJ (A) or LJ + n - 6 (B)
DevStageArgs stage_args(int n, int stage, const WideDevSites& sites, const double4* gates, const double2* cs, int E) {
    DevStageArgs a{};
    a.gates = gates; a.cs = cs; a.E = E;
    for (int l = 0; l < 6; ++l) {
        const int q = stage == 0 || l < 2 ? l : l + n - 6, j = stage == 0 ? l : l + n - 6;
        for (int k = 0; k < 4; ++k) element_form(sites.at(k, q), a.chan[k][l]);
        slot_form(sites.lam2[j], a.keep2[l], a.mix2[l]);
    }
    return a;
}

struct DevWideCall {
    DevStageArgs stage[2];
    DensArgs out;                           // what the read-out kernel reads: pred, sd, bias
    long B;
    int nb[2], ld[2], pauli;
};

// every stage and the read-out of one call, in stream order
template <int N>
int launch_density_dev_wide(const DevWideCall& c, double2* rho, double* hv, hipStream_t st) {
    const dim3 grid((unsigned)(c.B << (2 * (N - 6)))), block(kDensThreads);
    int rc = QHEA_OK;
    bool first = true;
    auto ring = [&](int s, int col, bool enc) {
        rc = launch_dynamic_lds(density_dev_wide_ring_kernel<N, 0>, grid, block, kDensStateBytes, st, c.stage[0], rho, s, col,
                                (int)enc, (int)first);
        first = false;
        if (rc == QHEA_OK)
            rc = launch_dynamic_lds(density_dev_wide_ring_kernel<N, 1>, grid, block, kDensStateBytes, st, c.stage[1], rho, s, col,
                                    (int)enc, 0);
    };
    auto wires = [&](int col, int kind) {
        rc = launch_dynamic_lds(density_dev_wide_wires_kernel<N, 0>, grid, block, kDensStateBytes, st, c.stage[0], rho, col, kind,
                                (int)first);
        first = false;
        if (rc == QHEA_OK && kind != 3)
            rc = launch_dynamic_lds(density_dev_wide_wires_kernel<N, 1>, grid, block, kDensStateBytes, st, c.stage[1], rho, col,
                                    kind, 0);
    };
    int s = 0, col = 0;
    for (int g = 0; g < 2; ++g) {
        for (int b = 0; b < c.nb[g]; ++b) {
            if (c.ld[g] == 0) {
                wires(col, 0);
                if (rc != QHEA_OK) return rc;
            }
            for (int l = 0; l < c.ld[g]; ++l, ++s) {
                ring(s, col, l == 0);
                if (rc != QHEA_OK) return rc;
            }
            col += N;
        }
    }
    if (first) wires(0, 3);                                              // no block at all: rho = |0><0|
    if (rc == QHEA_OK && c.pauli != QHEA_PAULI_Z) wires(0, c.pauli == QHEA_PAULI_X ? 1 : 2);
    if (rc != QHEA_OK) return rc;
    hipLaunchKernelGGL(density_wide_readout_kernel<N>, dim3((unsigned)c.B), dim3(64), 0, st, c.out, rho, hv);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

}  // namespace
}  // namespace qhea
