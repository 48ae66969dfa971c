// hea_density_wide.hip -- qhea_model_forward_noisy_exact_wide: the exact noisy forward of hea_density.hip for n = 7, 8, 9, where
// a row's 4^n elements of rho (256 KiB, 1 MiB, 4 MiB) no longer fit in LDS.  rho of all rows of the call lives in the workspace,
// 4^n x 16 bytes per row, in hea_density.hip's index layout (bit 2q: wire q's row bit, bit 2q + 1: its column bit).
//
// A stage is one launch over rows x tiles.  A tile is the 4^6 elements that share the 2 (n - 6) index bits of the wires a stage
// leaves alone; a workgroup of 256 threads copies its tile into 64 KiB of LDS (the n = 6 slot layout and fold), runs passes of
// Pass<6, J> over it (16 elements per thread, one barrier per pass) and copies it back.  Two tilings serve every pass:
//   stage A: local wires (0, 1, 2, 3, 4, 5).  element i = tile << 12 | l: one contiguous 64 KiB block of the row.
//   stage B: local wires (0, 1, n-4, n-3, n-2, n-1).  element i = (l & 15) | tile << 4 | (l >> 4) << (2n - 8): runs of 16
//            contiguous elements (256 bytes).
// A sub-layer is stage A with the ring passes j = 0..4 (Pass<6, j>), then stage B with j = 5..n-1: the pair (j, j + 1) is the
// local pair (j - n + 6, j - n + 7) and the closing pair (n - 1, 0) the local pair (5, 0), Pass<6, j - n + 6>.  The pending-gate
// rule is hea_density.hip's in global wires: pass 0 applies wire 0's gates, every pass j <= n - 2 wire j + 1's, pass n - 1 none.
// Blocks without sub-layers and the basis change of the X / Y read-outs are one-qubit stages on the same tiles: stage A serves
// wires 0..5, stage B wires 6..n-1 only.  The first stage of a circuit loads nothing: tile 0 starts from |0><0|, the others
// from zero.
//
// The launch boundary is the only synchronisation between the tiles of a row: no workgroup waits on another, stream order
// carries a stage's stores to the next.  The copy between global memory and LDS is a phase of its own in which consecutive
// lanes take consecutive elements of a run.
//
// Read-out: one small kernel per call writes h'[2^n] and h2'[2^n] (the value table and its square under the readout
// confusion, n two-point mixes) to the workspace; a wave per row adds p_k h'[k] and p_k h2'[k] over diag rho: lane l the terms
// k = l + 64 r in the order r = 0, 1, .., then the 64 lane sums by the xor butterfly, offsets 32, 16, .. 1.  No atomics, nothing
// depends on the batch or on other rows: a row's results are bitwise the same in any call.
//
// The tile maps, the copy phase, the read-out kernel, the workspace layout and the dispatch on n are hea_density_wide.hpp's,
// shared with hea_density_device_wide.hip (the same stages under a calibrated device noise model).
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

using namespace qhea;

extern "C" {

size_t qhea_model_exact_noisy_wide_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (batch < 0 || model_info(desc, mi) != QHEA_OK || mi.n < 7 || mi.n > 9) return 0;
    return wide_layout(mi, batch).total;
}

int qhea_model_forward_noisy_exact_wide(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                                        const double* params, const double* ham_diag, const qhea_noise* noise, double* pred,
                                        double* shot_std, void* workspace, size_t workspace_bytes, void* stream) {
    NoisyCall c;
    int rc = noisy_call_check({7, 9 /* rho in the workspace, six wires at a time in LDS */, false, false}, desc, ham_diag, noise,
                              0, batch, trunk, {branch, params, pred}, workspace, stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    if (batch > (int64_t)INT_MAX >> (2 * (c.mi.n - 6))) return QHEA_EINVAL;     // a stage has one workgroup per (row, tile)
    const WideLayout L = wide_layout(c.mi, batch);
    if (!workspace || workspace_bytes < L.total) return QHEA_EWORKSPACE;
    double4* gates = reinterpret_cast<double4*>(c.ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(c.ws + L.off_cs);
    double* hv = reinterpret_cast<double*>(c.ws + L.off_hv);
    double2* rho = reinterpret_cast<double2*>(c.ws + L.off_rho);
    rc = launch_prep_model(desc, c.mi, batch, branch, trunk, params, gates, cs, c.ws, c.st);
    if (rc != QHEA_OK) return rc;

    DensArgs a = dens_args(desc, c.mi, noise, params, ham_diag, batch, gates, cs);
    a.pred = pred; a.sd = shot_std;
    hipLaunchKernelGGL(density_wide_values_kernel, dim3(1), dim3(512), 0, c.st, a, c.mi.n, hv);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    return dispatch_wide_n(c.mi.n, [&](auto n) { return launch_density_wide<n()>(a, rho, hv, c.st); });
}

}  // extern "C"
