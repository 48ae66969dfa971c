// hea_density_wide_grad.hpp -- what the two tiled density-matrix gradient units share (hea_density_wide_grad.hip: the uniform
// channels, hea_density_device_wide_grad.hip: the calibrated device noise model), n = 7, 8, 9: what a reverse-stage workgroup
// is, the reverse one-qubit stages (a block's encoding under the uniform channels; the daggers of the read-out basis change,
// which carry no noise), the O_N kernel, the fold of the per-tile trace partials and the workspace layout.
// hea_density_wide_grad.hip describes them.  Everything sits in an unnamed namespace: each unit compiles its own copy.
#pragma once
#include "hea_density_grad.hpp"
#include "hea_density_wide.hpp"

namespace qhea {
namespace {

constexpr int kTileElems = 4096;                                         // 4^6
// LDS of a reverse-stage workgroup: the tiles of rho and of O, two buffers of the four waves' trace partials
constexpr size_t kWideBwdLds = 2 * (size_t)kDensStateBytes + 2 * RowCtx<6>::WPR * kTracesPerPass * sizeof(double);

// What a reverse-stage workgroup is: its tile of rho and of O in LDS, and where its partials go -- flush_traces<6> writes
// a.rec[idx B' + r'] with B' = rows x tiles and r' = row x tiles + tile, which is partial[idx][row][tile]
template <int N>
__device__ __forceinline__ RowCtx<6> tile_ctx(double2* lds, int tid, long r, int tile, long B) {
    constexpr int TB = 2 * (N - 6);
    RowCtx<6> cx;
    cx.rho = lds;
    cx.obs = lds + kTileElems;
    cx.red = reinterpret_cast<double*>(lds + 2 * kTileElems);
    cx.rank = tid; cx.sf = 0; cx.parity = 0;
    cx.r = (r << TB) + tile; cx.B = B << TB; cx.live = true;
    return cx;
}

// the local wires (LJ, LJ + 1) of a tile in reverse, those of them the stage serves (wide_wire_pass' rule).  BASIS = false:
// a block's encoding (channel, trace, RX^dagger: the body of encoding_passes_back); true: the dagger of the read-out basis
// change on rho and O, kind 3 = H, 4 = S H (basis_passes_back's gates, no noise, no trace)
template <int N, int STAGE, int LJ, bool BASIS>
__device__ __forceinline__ void wide_wire_pass_back(RowCtx<6>& cx, const DensGradArgs& a, const double2* csr, int col, int kind) {
    constexpr int up = STAGE ? N - 6 : 0, served = STAGE ? 12 - N : 0;   // global wire = local + up; stage B: global >= 6
    constexpr bool T = LJ >= served, C = LJ + 1 >= served;
    if constexpr (T || C) {
        using P = Pass<6, LJ>;
        const int i0 = P::base(cx.rank | opaque_zero()), b = i0 ^ fold(i0);
        double2 e[16], o[16];
        P::load(e, cx.rho, b);
        P::load(o, cx.obs, b);
        if constexpr (BASIS) {
            const U2 h = kind == 3 ? U2{{M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {-M_SQRT1_2, 0.0}}
                                   : U2{{M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {0.0, M_SQRT1_2}, {0.0, -M_SQRT1_2}};
            if (T) { apply_gate<1>(e, h); apply_gate<1>(o, h); }
            if (C) { apply_gate<4>(e, h); apply_gate<4>(o, h); }
            P::store(e, cx.rho, b);
            P::store(o, cx.obs, b);
            __syncthreads();
        } else {
            double tr[kTracesPerPass];
            int idx[kTracesPerPass];
#pragma unroll
            for (int i = 0; i < kTracesPerPass; ++i) { tr[i] = 0.0; idx[i] = -1; }
            if (T) {
                undo_encoding<1>(e, o, a, csr[col + LJ + up], tr);
                idx[3] = col + LJ + up;
            }
            if (C) {
                undo_encoding<4>(e, o, a, csr[col + LJ + 1 + up], tr + 4);
                idx[7] = col + LJ + 1 + up;
            }
            P::store(e, cx.rho, b);
            P::store(o, cx.obs, b);
            flush_traces<6>(cx, a, tr, idx);
        }
    }
}

// a reverse one-qubit stage: stage A wires 0..5, stage B wires 6..n-1
template <int N, int STAGE, bool BASIS>
__global__ __launch_bounds__(kDensThreads) void density_wide_wires_back_kernel(DensGradArgs a, double2* rho, double2* obs,
                                                                               int col, int kind) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    double2* rrow = rho + ((size_t)r << (2 * N));
    double2* orow = obs + ((size_t)r << (2 * N));
    const double2* csr = a.f.cs + r * a.f.E;
    RowCtx<6> cx = tile_ctx<N>(lds, tid, r, tile, a.f.B);
    tile_load<N, STAGE>(cx.rho, rrow, tile, tid, false);
    tile_load<N, STAGE>(cx.obs, orow, tile, tid, false);
    wide_wire_pass_back<N, STAGE, 4, BASIS>(cx, a, csr, col, kind);
    wide_wire_pass_back<N, STAGE, 2, BASIS>(cx, a, csr, col, kind);
    wide_wire_pass_back<N, STAGE, 0, BASIS>(cx, a, csr, col, kind);
    tile_store<N, STAGE>(cx.rho, rrow, tile, tid);
    tile_store<N, STAGE>(cx.obs, orow, tile, tid);
}

// O_N = diag(h' - mean h') in the read-out basis, zero elsewhere.  One workgroup per (row, stage A tile): 4096 consecutive
// elements.  The mean: every wave adds h'[k], lane l the terms k = l + 64 r in the order r = 0, 1, .., then the butterfly
template <int N>
__global__ __launch_bounds__(kDensThreads) void density_wide_observable_kernel(const double* hv, double2* obs) {
    constexpr int TB = 2 * (N - 6), D = 1 << N;
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    double hbar = 0.0;
    for (int k = tid & 63; k < D; k += 64) hbar += hv[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) hbar += __shfl_xor(hbar, d);
    hbar *= 1.0 / D;
    double2* out = obs + (size_t)blockIdx.x * kTileElems;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int l = j * kDensThreads + tid;
        const unsigned i = (unsigned)tile << 12 | (unsigned)l;
        int k = 0;
        bool diag = true;
#pragma unroll
        for (int w = 0; w < N; ++w) {
            const int rb = (i >> (2 * w)) & 1, cb = (i >> (2 * w + 1)) & 1;
            diag = diag && rb == cb;
            k |= rb << w;
        }
        out[l] = make_double2(diag ? hv[k] - hbar : 0.0, 0.0);
    }
}

// rec[angle][row] = the partials of the row's tiles added in tile order; pred_ws to the caller's pred.  One thread per sum
__global__ __launch_bounds__(256) void density_wide_fold_kernel(const double* partial, double* rec, long nsum, int tiles,
                                                                const double* pred_ws, double* pred, long B) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < nsum) {
        const double* p = partial + i * tiles;
        double t = p[0];
        for (int k = 1; k < tiles; ++k) t += p[k];
        rec[i] = t;
    }
    if (pred && i < B) pred[i] = pred_ws[i];
}

// ---- host --------------------------------------------------------------------------------------------------------------------

struct WideGradLayout { size_t off_hv, off_partial, off_rho, off_obs, total; };

// dens_grad_layout's regions (prep tables, pred, records: what grad_launch hands out), then h' and h'^2, the partials and
// the two matrices
WideGradLayout wide_grad_layout(const ModelInfo& mi, int64_t B) {
    WideGradLayout L{};
    const size_t nrec = (size_t)mi.sh.E + (size_t)3 * mi.n * mi.sh.blk, mat = ((size_t)B << (2 * mi.n)) * sizeof(double2);
    size_t p = dens_grad_layout(mi, B).total;
    L.off_hv = p;      p = align256(p + ((size_t)2 << mi.n) * sizeof(double));
    L.off_partial = p; p = align256(p + ((size_t)B << (2 * (mi.n - 6))) * nrec * sizeof(double));
    L.off_rho = p;     p = align256(p + mat);
    L.off_obs = p;     p = align256(p + mat);
    L.total = p;
    return L;
}

}  // namespace
}  // namespace qhea
