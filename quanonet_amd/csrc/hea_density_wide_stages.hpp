// hea_density_wide_stages.hpp -- the stages of the exact noisy forward at n = 7, 8, 9 under the uniform channels: the ring and
// one-qubit stage kernels, the value-table kernel and launch_density_wide, the launch sequence of one call.  hea_density_wide.hip
// describes them and is their entry point; hea_density_wide_grad.hip runs the same sequence as the forward sweep of the adjoint
// gradient, so that its pred is the forward's bit for bit.  A header of its own, not part of hea_density_wide.hpp: the value
// table kernel is no template, and hea_density_device_wide.hip (which includes that header) must not grow a kernel it never
// launches.  Everything sits in an unnamed namespace: each unit compiles its own copy into its own kernels.
#pragma once
#include "hea_density_wide.hpp"

namespace qhea {
namespace {

// ring pass J of the circuit's n wires on the tile that holds both of its wires
template <int N, int J>
__device__ __forceinline__ void wide_ring_pass(double2* lds, int rank, const DensArgs& a, const double2* csr, int s, int col,
                                               bool enc) {
    using P = Pass<6, (J < 5 ? J : J - N + 6)>;
    const int i0 = P::base(rank), b = i0 ^ fold(i0);
    double2 e[16];
    P::load(e, lds, b);
    if (J == 0) wire_gates<N, 1>(e, a, csr, s, col, enc, 0);
    if (J <= N - 2) wire_gates<N, 4>(e, a, csr, s, col, enc, J + 1);
    cnot_depolarize2(e, a.d2_keep, a.d2_mix);
    P::store(e, lds, b);
    __syncthreads();
}
template <int N, int J, int JEND>
__device__ __forceinline__ void wide_ring_passes(double2* lds, int rank, const DensArgs& a, const double2* csr, int s, int col,
                                                 bool enc) {
    if constexpr (J < JEND) {
        wide_ring_pass<N, J>(lds, rank, a, csr, s, col, enc);
        wide_ring_passes<N, J + 1, JEND>(lds, rank, a, csr, s, col, enc);
    }
}

// a ring stage of sub-layer s: stage A passes 0..4, stage B passes 5..n-1.  Grid: rows x 4^(n-6) workgroups, tile fastest
template <int N, int STAGE>
__global__ __launch_bounds__(kDensThreads) void density_wide_ring_kernel(DensArgs a, double2* rho, int s, int col, int enc,
                                                                         int first) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    double2* row = rho + ((size_t)r << (2 * N));
    const double2* csr = a.cs + r * a.E;
    tile_load<N, STAGE>(lds, row, tile, tid, first != 0);
    if (STAGE == 0) wide_ring_passes<N, 0, 5>(lds, tid, a, csr, s, col, enc != 0);
    else wide_ring_passes<N, 5, N>(lds, tid, a, csr, s, col, enc != 0);
    tile_store<N, STAGE>(lds, row, tile, tid);
}

// one-qubit gates on the local wires (LJ, LJ + 1) of a tile, those of them the stage serves: kind 0 = a block's encoding RX
// with its channel, 1 = H, 2 = H S^dagger (read-out basis, no noise)
template <int N, int STAGE, int LJ>
__device__ __forceinline__ void wide_wire_pass(double2* lds, int rank, const DensArgs& a, const double2* csr, int col, int kind) {
    constexpr int up = STAGE ? N - 6 : 0, served = STAGE ? 12 - N : 0;   // global wire = local + up; stage B: global >= 6
    constexpr bool T = LJ >= served, C = LJ + 1 >= served;
    if constexpr (T || C) {
        using P = Pass<6, LJ>;
        const int i0 = P::base(rank), b = i0 ^ fold(i0);
        double2 e[16];
        P::load(e, lds, b);
        const U2 h = kind == 1 ? U2{{M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {-M_SQRT1_2, 0.0}}
                               : U2{{M_SQRT1_2, 0.0}, {0.0, -M_SQRT1_2}, {M_SQRT1_2, 0.0}, {0.0, M_SQRT1_2}};
        if (T) {
            apply_gate<1>(e, kind == 0 ? encoding_rx(csr[col + LJ + up]) : h);
            if (kind == 0) depolarize1<1>(e, a);
        }
        if (C) {
            apply_gate<4>(e, kind == 0 ? encoding_rx(csr[col + LJ + 1 + up]) : h);
            if (kind == 0) depolarize1<4>(e, a);
        }
        P::store(e, lds, b);
        __syncthreads();
    }
}

// a one-qubit stage: stage A wires 0..5, stage B wires 6..n-1; kind 3 = no gate at all (a circuit without blocks: stage A
// with `first` writes rho = |0><0|)
template <int N, int STAGE>
__global__ __launch_bounds__(kDensThreads) void density_wide_wires_kernel(DensArgs a, double2* rho, int col, int kind,
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
        wide_wire_pass<N, STAGE, 0>(lds, tid, a, csr, col, kind);
        wide_wire_pass<N, STAGE, 2>(lds, tid, a, csr, col, kind);
        wide_wire_pass<N, STAGE, 4>(lds, tid, a, csr, col, kind);
    }
    tile_store<N, STAGE>(lds, row, tile, tid);
}

// value tables under the readout confusion: n two-point mixes of h and h^2; hv = h'[2^n], then h2'[2^n].  One workgroup
__global__ __launch_bounds__(512) void density_wide_values_kernel(DensArgs a, int n, double* hv) {
    __shared__ double sh[2 * 512];
    const int tid = threadIdx.x, D = 1 << n;
    double h = 0.0, h2 = 0.0;
    if (tid < D) {
        h = a.diag ? a.diag[tid] : a.off + a.co * (double)(n - 2 * (int)__popc(tid));
        h2 = h * h;
    }
    for (int i = 0; i < n; ++i) {
        if (tid < D) { sh[tid] = h; sh[D + tid] = h2; }
        __syncthreads();
        if (tid < D) {
            h = (1.0 - a.q) * h + a.q * sh[tid ^ (1 << i)];
            h2 = (1.0 - a.q) * h2 + a.q * sh[D + (tid ^ (1 << i))];
        }
        __syncthreads();
    }
    if (tid < D) { hv[tid] = h; hv[D + tid] = h2; }
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// every stage and the read-out of one call, in stream order
template <int N>
int launch_density_wide(const DensArgs& a, double2* rho, double* hv, hipStream_t st) {
    const dim3 grid((unsigned)(a.B << (2 * (N - 6)))), block(kDensThreads);
    int rc = QHEA_OK;
    bool first = true;
    auto ring = [&](int s, int col, bool enc) {
        rc = launch_dynamic_lds(density_wide_ring_kernel<N, 0>, grid, block, kDensStateBytes, st, a, rho, s, col, (int)enc,
                                (int)first);
        first = false;
        if (rc == QHEA_OK)
            rc = launch_dynamic_lds(density_wide_ring_kernel<N, 1>, grid, block, kDensStateBytes, st, a, rho, s, col, (int)enc, 0);
    };
    auto wires = [&](int col, int kind) {
        rc = launch_dynamic_lds(density_wide_wires_kernel<N, 0>, grid, block, kDensStateBytes, st, a, rho, col, kind, (int)first);
        first = false;
        if (rc == QHEA_OK && kind != 3)
            rc = launch_dynamic_lds(density_wide_wires_kernel<N, 1>, grid, block, kDensStateBytes, st, a, rho, col, kind, 0);
    };
    int s = 0, col = 0;
    for (int g = 0; g < 2; ++g) {
        for (int b = 0; b < a.nb[g]; ++b) {
            if (a.ld[g] == 0) {
                wires(col, 0);
                if (rc != QHEA_OK) return rc;
            }
            for (int l = 0; l < a.ld[g]; ++l, ++s) {
                ring(s, col, l == 0);
                if (rc != QHEA_OK) return rc;
            }
            col += N;
        }
    }
    if (first) wires(0, 3);                                              // no block at all: rho = |0><0|
    if (rc == QHEA_OK && a.pauli != QHEA_PAULI_Z) wires(0, a.pauli == QHEA_PAULI_X ? 1 : 2);
    if (rc != QHEA_OK) return rc;
    hipLaunchKernelGGL(density_wide_readout_kernel<N>, dim3((unsigned)a.B), dim3(64), 0, st, a, rho, hv);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

}  // namespace
}  // namespace qhea
