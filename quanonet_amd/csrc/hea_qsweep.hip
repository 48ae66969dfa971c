// hea_qsweep.hip -- the backward kernel of ONE register class of qubit sweeps (compile with -DQHEA_CLASS=<c>, hea_qsweep.hpp;
// one object per class keeps the build parallel).  A workgroup takes its (member, sample group) from the class's work list,
// reads the member's n, depths and read-out from its MemberRec with scalar loads and runs the packed backward body of that n:
// per member the arithmetic and summation order of bwd_kernel<n, MINW, DepthArgs>.
#include "hea_qsweep.hpp"

#ifndef QHEA_CLASS
#error "compile with -DQHEA_CLASS=<register class>"
#endif
#define QHEA_CAT_(a, b) a##b
#define QHEA_CAT(a, b) QHEA_CAT_(a, b)

namespace qhea {

// The packed backward kernel's work on sample group grp (kWaves waves) -- bwd_kernel's body (hea_device.hpp) as a device function
// with the LDS passed in: forward sweep, psi / lambda walked back through the sub-layers, per-wave partial sums of the ansatz
// gradients, encoding gradients, in bwd_kernel's order of operations.  (bwd_kernel keeps its own copy: calling this from it
// changes the n = 9 kernel's register allocation, 44 instead of 41 AGPRs.)  MEM: block counts dc (a sweep member's) instead of
// the run table's.  cs_lds: kWaves * kCsPerWave + 16 pairs; red_lds: kWaves * Cfg<N>::REDW doubles where Cfg<N>::LDSRED;
// gate_ring: kWaves * kRingBytesPerWave bytes.
template <int N, bool MEM>
__device__ __forceinline__ void bwd_packed_body(long grp, const Runs& runs, const DepthCounts& dc, long B, int E, int blk,
                                                const double2* __restrict__ cs, const char* __restrict__ gates, int gates_bytes,
                                                double off, double co, const double* __restrict__ diag, int pauli,
                                                const double* __restrict__ g, const double* __restrict__ state_in,
                                                const double* __restrict__ y, const double* __restrict__ bias, double inv_bt,
                                                double* __restrict__ out, double* __restrict__ grad_x, double* __restrict__ partial,
                                                double2* cs_lds, double* red_lds, char* gate_ring) {
    using C = Cfg<N>;
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;         // (scalarising it costs the n = 8 kernel 3 %: measured)
    double* red = red_lds + (C::LDSRED ? wib * C::REDW : 0);
    const long wave = grp * kWaves + wib;
    const long b_raw = wave * C::SPW + (lane >> C::LB);
    const bool valid = b_raw < B;
    const long b = valid ? b_raw : B - 1;
    const int klow = lane & (C::LANES - 1);
    const int ring_fwd = ring_source<N>(lane, false);
    const int ring_rev = ring_source<N>(lane, true);

    CsStream<N> csx;
    csx.init(cs_lds + wib * kCsPerWave, cs, b, E, lane, lane >> C::LB);
    GateStream<N> gs;
    gs.init(gates, gates_bytes, gate_ring + wib * kRingBytesPerWave, lane);

    double pr[C::R], pi[C::R], lr[C::R], li[C::R];
    if (state_in) {
#pragma unroll
        for (int r = 0; r < C::R; ++r) {
            const double2 a = reinterpret_cast<const double2*>(state_in)[(b << N) + ((r << C::LB) | klow)];
            pr[r] = a.x; pi[r] = a.y;
        }
    } else {
        forward_sweep<N, MEM>(pr, pi, runs, csx, gs, lane, ring_fwd, dc);
    }

    basis_change<N, false>(pr, pi, pauli, lane);
    // upstream weight: given (g), or the fused MSE residual 2 (out + bias - y) / batch_total when y != NULL
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < C::R; ++r)
        acc += ham_weight<N>((r << C::LB) | klow, off, co, diag) * (pr[r] * pr[r] + pi[r] * pi[r]);
    double gb;
    if (y || out) {
        double v[1] = {acc};
        lane_reduce<1, C::LB>(v, lane);                      // butterfly: every lane of the sample gets the sum
        const double pred = v[0] + (bias ? bias[0] : 0.0);
        if (out && valid && klow == 0) out[b] = pred;
        gb = y ? 2.0 * (pred - y[b]) * inv_bt : g[b];
    } else {
        gb = g[b];
    }
    if (!valid) gb = 0.0;                                    // padding lanes carry lambda = 0: no gradient contribution
#pragma unroll
    for (int r = 0; r < C::R; ++r) {
        const double h = ham_weight<N>((r << C::LB) | klow, off, co, diag);
        lr[r] = gb * h * pr[r];
        li[r] = gb * h * pi[r];
    }
    if (pauli) {
        basis_change<N, true>(pr, pi, pauli, lane);
        basis_change<N, true>(lr, li, pauli, lane);
    }

    double* __restrict__ part_w = partial + wave * (long)blk * C::KW;
    GradSums<N> sums;
    sums.sub_w = -1; sums.col_x = -1; sums.m_x = 0; sums.red = red; sums.lane = lane; sums.wave = wave; sums.B = B;
    sums.E = E; sums.part_w = part_w; sums.grad_x = grad_x;
    int col = E, sub = blk;
    gs.template prime<false>(blk - 1);
    for (int ri = runs.nruns - 1; ri >= 0; --ri) {
        const int ne = runs.enc[ri], nld = runs.ld[ri];
        const bool one_chunk = ne <= N;
        const bool fold = kFold<N> && nld > 0 && ne > 0;   // the block's first RX chunk rides on sub-layer 0's gates
        const int m0 = ne < N ? ne : N;
        for (int rep = 0; rep < run_count<MEM>(runs, ri, dc); ++rep) {
            if (one_chunk && !fold && ne > 0) csx.template prefetch<false>(col - ne);   // this block's angles, used after its sub-layers
            for (int l = nld - 1; l >= 0; --l) {
                --sub;
                const bool folded = fold && l == 0;
                if constexpr (kFold<N>) {
                    if (folded) {
                        csx.template need<false>(col - ne, m0);
                        gs.template fold<false>(csx, col - ne, m0, lane);
                    }
                }
                apply_ring<N, true>(pr, pi, lane, ring_rev);
                apply_ring<N, true>(lr, li, lane, ring_rev);
                double acc3[C::KW];
#pragma unroll
                for (int i = 0; i < C::KW; ++i) acc3[i] = 0.0;
                gs.template begin<false>();
                static_rfor<0, N>([&](auto q) {
                    constexpr int Q = decltype(q)::value;
                    const double4 u = gs.template cur<false, Q>();
                    su2_inverse_with_inner<N, Q>(pr, pi, lr, li, u, lane, acc3[3 * Q], acc3[3 * Q + 1], acc3[3 * Q + 2]);
                    gs.template done<false, Q>();
                });
                gs.template advance<false>();
                if constexpr (C::LDSRED) {
                    sums.put_w(acc3, sub);
                } else {
                    const int vi = butterfly_sum<C::KW>(acc3, lane);   // the sample's total of value vi (cheapest lane-bit order)
                    if (butterfly_owner<C::KW>(lane)) part_w[(long)sub * C::KW + vi] = acc3[0];
                    if constexpr (kFold<N>) {
                        if (folded) {                                // encoding gradients of the folded chunk: n . (X,Y,Z)
                            const int q = vi / 3;                    // the lane holding X_q fetches Y_q and Z_q
                            const double Y = __shfl(acc3[0], butterfly_lane_of<C::KW>(vi + 1 < C::KW ? vi + 1 : vi));
                            const double Z = __shfl(acc3[0], butterfly_lane_of<C::KW>(vi + 2 < C::KW ? vi + 2 : vi));
                            if (butterfly_owner<C::KW>(lane) && vi % 3 == 0 && q < m0 && valid) {
                                const double4 ub = *reinterpret_cast<const double4*>(gates + ((long)(sub + 1) * N + q) * kGateBytes);
                                double nx, ny, nz;
                                rotated_x_axis(ub, nx, ny, nz);
                                grad_x[b * E + (col - ne) + q] = nx * acc3[0] + ny * Y + nz * Z;
                            }
                        }
                    }
                }
            }
            col -= ne;
            if (fold) {
                const int nchunks = (ne + N - 1) / N;
                for (int ch = nchunks - 1; ch >= 1; --ch) {          // chunk 0 was folded
                    const int j0 = ch * N;
                    const int m = (ne - j0) < N ? (ne - j0) : N;
                    csx.template need<false>(col + j0, m);
                    double gx[C::KX];
#pragma unroll
                    for (int i = 0; i < C::KX; ++i) gx[i] = 0.0;
                    static_rfor<0, N>([&](auto q) {
                        constexpr int Q = decltype(q)::value;
                        if (Q < m) {
                            const double2 c = csx.at(col + j0 + Q);
                            gx[Q] = pauli_x_inner<N, Q>(pr, pi, lr, li);
                            apply_rx<N, Q>(pr, pi, c.x, -c.y);
                            apply_rx<N, Q>(lr, li, c.x, -c.y);
                        }
                    });
                    store_grad_x<N>(gx, lane, wave, B, E, grad_x, col + j0, m);
                }
            } else if (one_chunk) {
                if (ne > 0) {
                    double gx[C::KX];
#pragma unroll
                    for (int i = 0; i < C::KX; ++i) gx[i] = 0.0;
                    rfor_gates_below<N>(ne, [&](auto q) {
                        constexpr int Q = decltype(q)::value;
                        gx[Q] = pauli_x_inner<N, Q>(pr, pi, lr, li);
                        apply_rx<N, Q>(pr, pi, csx.nxt[Q].x, -csx.nxt[Q].y);
                        apply_rx<N, Q>(lr, li, csx.nxt[Q].x, -csx.nxt[Q].y);
                    });
                    if constexpr (C::LDSRED) sums.put_x(gx, col, ne);
                    else store_grad_x<N>(gx, lane, wave, B, E, grad_x, col, ne);
                }
            } else {
                const int nchunks = (ne + N - 1) / N;
                for (int ch = nchunks - 1; ch >= 0; --ch) {
                    const int j0 = ch * N;
                    const int m = (ne - j0) < N ? (ne - j0) : N;
                    csx.template need<false>(col + j0, m);
                    double gx[C::KX];
#pragma unroll
                    for (int i = 0; i < C::KX; ++i) gx[i] = 0.0;
                    static_rfor<0, N>([&](auto q) {
                        constexpr int Q = decltype(q)::value;
                        if (Q < m) {
                            const double2 c = csx.at(col + j0 + Q);
                            gx[Q] = pauli_x_inner<N, Q>(pr, pi, lr, li);
                            apply_rx<N, Q>(pr, pi, c.x, -c.y);
                            apply_rx<N, Q>(lr, li, c.x, -c.y);
                        }
                    });
                    if constexpr (C::LDSRED) sums.put_x(gx, col + j0, m);
                    else store_grad_x<N>(gx, lane, wave, B, E, grad_x, col + j0, m);
                }
            }
        }
    }
    if constexpr (C::LDSRED) { sums.flush_w(); sums.flush_x(); }
}


// doubles of red_lds for the class: the largest Cfg<N>::LDSRED footprint of its n
template <int NLO, int NHI>
constexpr int qs_red_doubles() {
    int r = 1;
    for (int n = NLO; n <= NHI; ++n)
        if (n <= 5 && kWaves * padded_3n(n) * 66 > r) r = kWaves * padded_3n(n) * 66;     // (Cfg<n>::REDW = KW x 66)
    return r;
}

template <int NLO, int NHI, int MINW>
__global__ __launch_bounds__(kWaves * 64, MINW) void bwd_qsweep_kernel(QubitBwdArgs a) {
    static_assert(qs_red_doubles<NLO, NHI>() >= (Cfg<NLO>::LDSRED ? kWaves * Cfg<NLO>::REDW : 1), "red_lds sizing");
    // LDS declared once for the class (per-n arrays in the cases would be allocated side by side)
    __shared__ double2 cs_lds[kWaves * kCsPerWave + 16];   // +16: slack for the unclamped prefetch
    __shared__ double red_lds[qs_red_doubles<NLO, NHI>()];
    __shared__ __attribute__((aligned(16))) char gate_ring[kWaves * kRingBytesPerWave];
    const int2 ent = qs_entry(a.wk, a.ms.ws, (int)blockIdx.x);
    const long m = ent.x, grp = ent.y;
    const long wsb = m * a.ms.ws;
    const ConstMemberRec mr = (ConstMemberRec)member_ptr(reinterpret_cast<const MemberRec*>(a.mrec), wsb);
    const int n = mr->nq;                                       // (workgroup-uniform: one member per workgroup)
    static_for<NLO, NHI + 1>([&](auto q) {
        constexpr int N = decltype(q)::value;
        if constexpr (qs_built(N)) {
            if (n == N && grp * kWaves < qs_nwaves(N, a.B)) {   // (groups past a short batch's last have no samples)
                const Runs& runs = a.runs[N - 2];
                const DepthCounts dc{mr->depth[0], mr->depth[1]};
                const int E = N * (dc.c0 + dc.c1);
                const int blk = dc.c0 * runs.ld[0] + dc.c1 * runs.ld[1];
                bwd_packed_body<N, true>(grp, runs, dc, a.B, E, blk,
                                         reinterpret_cast<const double2*>(reinterpret_cast<const char*>(a.cs) + wsb), a.gates + wsb,
                                         (blk + 2) * N * kGateBytes, mr->off, mr->co, mr->diag, mr->pauli, nullptr, nullptr,
                                         a.y + m * a.ms.rows, a.bias ? a.bias + m * a.ms.params : nullptr, a.inv_bt,
                                         reinterpret_cast<double*>(reinterpret_cast<char*>(a.out) + wsb),
                                         reinterpret_cast<double*>(reinterpret_cast<char*>(a.grad_x) + wsb),
                                         reinterpret_cast<double*>(reinterpret_cast<char*>(a.partial) + wsb),
                                         cs_lds, red_lds, gate_ring);
            }
        }
    });
}

void QHEA_CAT(launch_bwd_qsweep_, QHEA_CLASS)(dim3 grid, hipStream_t st, const QubitBwdArgs& a) {
    hipLaunchKernelGGL((bwd_qsweep_kernel<qs_class_lo(QHEA_CLASS), qs_class_hi(QHEA_CLASS), 1>), grid, dim3(kWaves * 64), 0, st, a);
}

}  // namespace qhea
