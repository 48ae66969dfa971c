// hea_density_wide.hpp -- what the two tiled density-matrix units share (hea_density_wide.hip: the uniform channels,
// hea_density_device_wide.hip: the calibrated device noise model), n = 7, 8, 9: the two tile index maps, the copy phase between
// global memory and LDS, the read-out kernel, the workspace layout and the dispatch on the qubit count.  hea_density_wide.hip
// describes the tiles and the stages.  Everything sits in an unnamed namespace, as in hea_density.hpp: each translation unit
// compiles its own copy into its own kernels.
#pragma once
#include "hea_density.hpp"

namespace qhea {
namespace {

// element of the row that local element l of `tile` is, for stage A (STAGE = 0) and stage B (1)
template <int N, int STAGE>
__device__ __forceinline__ size_t tile_element(int tile, int l) {
    if (STAGE == 0) return (size_t)tile << 12 | (size_t)l;
    return (size_t)(l & 15) | (size_t)tile << 4 | (size_t)(l >> 4) << (2 * N - 8);
}

// the copy phase: element l = 256 k + tid, so that a wave's lanes cover four runs of 16 elements (stage B) or one of 64 (A)
template <int N, int STAGE>
__device__ __forceinline__ void tile_load(double2* lds, const double2* row, int tile, int tid, bool first) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int l = k * kDensThreads + tid;
        lds[l ^ fold(l)] = first ? make_double2(l == 0 && tile == 0 ? 1.0 : 0.0, 0.0) : row[tile_element<N, STAGE>(tile, l)];
    }
    __syncthreads();
}
template <int N, int STAGE>
__device__ __forceinline__ void tile_store(const double2* lds, double2* row, int tile, int tid) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int l = k * kDensThreads + tid;
        row[tile_element<N, STAGE>(tile, l)] = lds[l ^ fold(l)];
    }
}

// read-out: one wave per row over diag rho; of `a` it reads pred, sd and bias
template <int N>
__global__ __launch_bounds__(64) void density_wide_readout_kernel(DensArgs a, const double2* rho, const double* hv) {
    constexpr int D = 1 << N;
    const int lane = threadIdx.x;
    const long r = blockIdx.x;
    const double2* row = rho + ((size_t)r << (2 * N));
    double m1 = 0.0, m2 = 0.0;
    for (int k = lane; k < D; k += 64) {
        unsigned i = 0;
#pragma unroll
        for (int w = 0; w < N; ++w) i |= ((k >> w) & 1) * (3u << (2 * w));
        const double p = row[i].x;
        m1 += p * hv[k];
        m2 += p * hv[D + k];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        m1 += __shfl_xor(m1, d);
        m2 += __shfl_xor(m2, d);
    }
    if (lane == 0) {
        a.pred[r] = m1 + (a.bias ? a.bias[0] : 0.0);
        if (a.sd) {
            const double var = m2 - m1 * m1;
            a.sd[r] = var > 0.0 ? sqrt(var) : 0.0;
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------

struct WideLayout { size_t off_gates, off_cs, off_hv, off_rho, total; };

WideLayout wide_layout(const ModelInfo& mi, int64_t B) {
    const TableLayout t = table_layout(mi, B);
    WideLayout L{};
    L.off_gates = t.off_gates; L.off_cs = t.off_cs;
    size_t p = t.end;
    L.off_hv = p;  p = align256(p + ((size_t)2 << mi.n) * sizeof(double));
    L.off_rho = p; p = align256(p + ((size_t)B << (2 * mi.n)) * sizeof(double2));
    L.total = p;
    return L;
}

template <class F>
int dispatch_wide_n(int n, F&& f) {
    switch (n) {
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 9: return f(std::integral_constant<int, 9>{});
        default: return QHEA_EUNSUPPORTED;
    }
}

}  // namespace
}  // namespace qhea
