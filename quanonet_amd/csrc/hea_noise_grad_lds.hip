// hea_noise_grad_lds.hip -- qhea_model_loss_grad_noisy_lds / qhea_model_train_steps_noisy_lds: the sampled-trajectory gradient of
// hea_noise_grad.hip for n = 10..12, where psi and lambda no longer fit a wave's registers.  Same quantity, estimator, random
// stream and record form (include/quanonet_hea.h); what differs is where the states live and, with it, the order of the sums.
//
// noisy_grad_lds_kernel<N>: one workgroup per (row, tile of kLdsGradTile trajectories); psi and lambda rest in LDS in the layout
// LCfg<N, LG> of hea_lds.hpp, LG = kGradLG<N> gate qubits per pass and 2^(n-LG) threads: 128 / 256 / 256 threads at n = 10 / 11 /
// 12 (n = 12: 2 x 64 KB of the CU's 160 KB + 2 KB of scratch, hence one workgroup per CU).  Per trajectory:
//   forward   the walk of noisy_wide_lds_kernel in this layout (noisy_layer): RX as a layer of its own, then per sub-layer the
//             fused gates and the ring; a segment's frame rides on its last pass's store (store_framed).  Wave 0 draws the
//             segment's Philox words and builds the frame (enc_frame / sub_frame), thread 0 hands it over in sc->frame;
//   read-out  behind the basis change thread t holds the 2^LG basis states from 2^LG t on: v = sum p_k h'(k) in that order, then
//             the wave by the xor butterfly, then the waves in wave order (at n = 12 the forward LDS kernel's order, at n = 10
//             and 11 groups of 8 where it has 16); lambda = h' psi; both back through the basis change's dagger;
//   reverse   per segment, last to first, on psi and lambda together: the frame again and the inverse ring in the first gather
//             (load_framed, the mirror of the forward's store), then per wire the inner products and the adjoint gate
//             (bwd_layer).  The frames are recomputed from the stream, not kept.
// Barriers of a reverse segment.  bwd_layer's pass 0 ends in a workgroup barrier, so a segment's last store is complete when the
// next segment begins.  Thread 0 then writes the next frame, and the barrier marked (F) below makes it visible before the
// gather that reads it; the frame's previous readers are a whole layer of barriers back.  The barrier inside bwd_layer's first
// pass keeps every gather ahead of the first store (the framed gather leaves the thread's own slots).
// Sums: the 3n (or n) per-thread values go over the wave by lane_reduce, the waves in wave order through sc->red, as in
// lds_bwd_kernel; thread i < 3n (or n) then adds value i to the item's record in global memory -- the first trajectory of the
// tile stores, later ones read, add and store, the same thread every time, so program order is all the ordering there is.  No
// atomics.  The fold and reduce launches behind the kernel are hea_noise_grad.hip's and hea_density_grad.hip's.
#include "hea_lds.hpp"
#include "hea_noise_grad.hpp"

namespace qhea {
namespace {

// Trajectories per work item: part of the stated summation order.  A workgroup walks its trajectories one after another, so a
// small batch wants many small items: measured at T = 64 (ms per step), tiles of 2 / 4 / 8 / 16 take 8.4 / 9.8 /
// 9.8 / 17.0 at Q10 batch 100, 78 / 84 / 97 / 96 on the cfg 5 model at batch 100 and 772 / 770 / 770 / 767 at its shard of 1024.
// The price of a small tile is the workspace: one record of E + 3 n blk doubles per tile.  The override is for that sweep.
#ifndef QHEA_NOISE_GRAD_LDS_TILE
#define QHEA_NOISE_GRAD_LDS_TILE 2
#endif
constexpr int kLdsGradTile = QHEA_NOISE_GRAD_LDS_TILE;

template <int NW>
struct GradScratch {                        // behind the two states
    double red[NW * 64];                    // per-wave sums
    int frame[2];                           // the segment's frame: phys(x), and z pulled back through the ring where there is one
    int pad[2];
};

// Gate qubits per pass: the backward layout's 3 at n = 10, 11.  At n = 12 that layout's 512 threads leave a thread 256 registers,
// which lds_bwd_kernel just fits (248) and this kernel, with the frame, the tile loop and the record on top, does not (28 VGPRs
// spilled to scratch in the cross-compile's report).  So n = 12 takes 4: 256 threads, one wave per SIMD, the register file of a
// SIMD to one wave (256 VGPRs + 170 AGPRs, no scratch), three passes per layer instead of four -- the trade hea_lds.hpp measured
// as even for the ideal backward kernel.
template <int N>
constexpr int kGradLG = N == 12 ? 4 : kBwdLG;

template <int N>
__global__ __launch_bounds__((LCfg<N, kGradLG<N>>::T)) void noisy_grad_lds_kernel(NoisyGradArgs g) {
    constexpr int LG = kGradLG<N>, M = 1 << LG;
    using L = LCfg<N, LG>;
    constexpr int KW = L::KW;
    extern __shared__ __attribute__((aligned(16))) char grad_lds[];
    double2* psi = reinterpret_cast<double2*>(grad_lds);
    double2* lam = psi + L::DIM;
    GradScratch<L::NW>* sc = reinterpret_cast<GradScratch<L::NW>*>(grad_lds + 2 * L::STATE_BYTES);
    const NoiseArgs& a = g.f;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long item = blockIdx.x;
    const long r = item / a.tiles, t0 = (item - r * a.tiles) * (long)kLdsGradTile;
    const int tcount = (int)(a.T - t0 < kLdsGradTile ? a.T - t0 : kLdsGradTile);
    const unsigned long long row = (unsigned long long)(a.row0 + r);
    const double2* csr = a.cs + r * a.E;
    double* rec = g.items + item * (long)g.width;
    double* rec_w = rec + a.E;
    Bases<N, LG> bs;
    bs.init(t);
    const int tpl = thread_part<Pass<N, L::NP - 1, LG>::A, LG>(t);
    const double off_term = g.hd ? 0.0 : a.off;
    constexpr double kR = 0.70710678118654752440;

    double sum = 0.0, sq = 0.0;
    for (int tj = 0; tj < tcount; ++tj) {
        const unsigned traj = (unsigned)(t0 + tj);
        const bool first = tj == 0;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int p = t + j * L::T;
            psi[p] = make_double2(p == 0 ? 1.0 : 0.0, 0.0);              // |0..0>: phys(0) = 0
        }
        __syncthreads();
        unsigned loc = 0;
        int s = 0, col = 0;
        for (int gi = 0; gi < 2; ++gi) {
            for (int b = 0; b < a.nb[gi]; ++b) {
                if (wave == 0) {
                    int x, z;
                    enc_frame<N>(segment_codes(a, loc, N, N, traj, row, lane), loc, x, z);
                    if (t == 0) { sc->frame[0] = phys<LG>(x); sc->frame[1] = z; }
                }
                noisy_layer<N, false, LG>(psi, bs, tpl, sc->frame, [&](int q) { return rx_su2(csr[col + q]); });
                col += N; loc += N;
                for (int l = 0; l < a.ld[gi]; ++l, ++s, loc += 2 * N) {
                    if (wave == 0) {
                        int x, z;
                        sub_frame<N>(segment_codes(a, loc, 2 * N, N, traj, row, lane), loc, x, z);
                        if (t == 0) { sc->frame[0] = phys<LG>(x); sc->frame[1] = ring_pull<N>(z); }
                    }
                    noisy_layer<N, true, LG>(psi, bs, tpl, sc->frame, [&](int q) { return a.gates[2 * ((s + 1) * N + q)]; });
                }
            }
        }
        // read-out: v over the thread's 2^LG consecutive basis states in order, lambda = h' psi
        if (a.pauli != QHEA_PAULI_Z) {                                   // same probabilities as H / H S^dagger
            const double4 ub = a.pauli == QHEA_PAULI_X ? make_double4(kR, 0.0, kR, 0.0) : make_double4(kR, 0.0, 0.0, -kR);
            if (t == 0) { sc->frame[0] = 0; sc->frame[1] = 0; }          // no frame behind the three basis layers
            noisy_layer<N, false, LG>(psi, bs, tpl, sc->frame, [&](int) { return ub; });
        }
        {
            c2 v[M], l[M];
            load_group<N, 0, false, LG>(psi, bs.plain[0], v);
            double val = 0.0;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const double hk = readout_weight<N>(a, g.hd, (t << LG) | j);
                val += (v[j].x * v[j].x + v[j].y * v[j].y) * hk;
                l[j].x = hk * v[j].x; l[j].y = hk * v[j].y;
            }
            store_group<N, 0, false, LG>(lam, bs.plain[0], l);
            val = wide_block_sum<L::NW>(val, sc->red) + off_term;
            sum += val; sq += val * val;
            __syncthreads();                                             // lambda is whole; sc->red is free again
        }
        if (a.pauli != QHEA_PAULI_Z) {
            const double4 ud = a.pauli == QHEA_PAULI_X ? make_double4(kR, 0.0, -kR, 0.0) : make_double4(kR, 0.0, 0.0, kR);
            noisy_layer<N, false, LG>(psi, bs, tpl, sc->frame, [&](int) { return ud; });
            noisy_layer<N, false, LG>(lam, bs, tpl, sc->frame, [&](int) { return ud; });
        }
        // reverse walk: blocks, sub-layers and wires in reverse order
        for (int gi = 1; gi >= 0; --gi) {
            for (int b = a.nb[gi] - 1; b >= 0; --b) {
                for (int l = a.ld[gi] - 1; l >= 0; --l) {
                    --s; loc -= 2 * N;
                    if (wave == 0) {
                        int x, z;
                        sub_frame<N>(segment_codes(a, loc, 2 * N, N, traj, row, lane), loc, x, z);
                        if (t == 0) { sc->frame[0] = phys<LG>(x); sc->frame[1] = ring_pull<N>(z); }
                    }
                    __syncthreads();                                     // (F) the frame is visible
                    double xyz[KW];
#pragma unroll
                    for (int i = 0; i < KW; ++i) xyz[i] = 0.0;
                    bwd_layer<N, LG, true, true, true>(psi, lam, bs, [&](int q, double4& u) {
                        u = dagger(a.gates[2 * ((s + 1) * N + q)]);
                        return true;
                    }, xyz, sc->frame, tpl);
                    lane_reduce<KW, 6>(xyz, lane);                       // lane i holds the wave total of value i
                    if (lane < KW) sc->red[wave * 64 + lane] = xyz[0];
                    __syncthreads();
                    if (t < 3 * N) {
                        double tot = sc->red[t];
#pragma unroll
                        for (int w = 1; w < L::NW; ++w) tot += sc->red[w * 64 + t];
                        double* p = rec_w + (long)s * 3 * N + t;
                        *p = first ? tot : *p + tot;
                    }
                }
                col -= N; loc -= N;
                if (wave == 0) {
                    int x, z;
                    enc_frame<N>(segment_codes(a, loc, N, N, traj, row, lane), loc, x, z);
                    if (t == 0) { sc->frame[0] = phys<LG>(x); sc->frame[1] = z; }
                }
                __syncthreads();                                         // (F) the frame is visible
                double gx[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) gx[i] = 0.0;
                bwd_layer<N, LG, false, false, true>(psi, lam, bs, [&](int q, double4& u) {
                    u = dagger(rx_su2(csr[col + q]));
                    return true;
                }, gx, sc->frame, tpl);
                lane_reduce<16, 6>(gx, lane);                            // lane l holds the wave total of value l & 15
                if (lane < 16) sc->red[wave * 64 + lane] = gx[0];
                __syncthreads();
                if (t < N) {
                    double tot = sc->red[t];
#pragma unroll
                    for (int w = 1; w < L::NW; ++w) tot += sc->red[w * 64 + t];
                    double* p = rec + col + t;
                    *p = first ? tot : *p + tot;
                }
            }
        }
    }
    if (t == 0) a.partial[item] = make_double2(sum, sq);
}

template <int N>
int launch_lds_n(const NoisyGradArgs& g, hipStream_t st) {
    using L = LCfg<N, kGradLG<N>>;
    constexpr size_t smem = 2 * L::STATE_BYTES + sizeof(GradScratch<L::NW>);
    return launch_dynamic_lds(noisy_grad_lds_kernel<N>, dim3((unsigned)(g.f.B * g.f.tiles)), dim3(L::T), smem, st, g);
}
// one workgroup per (row, tile)
int launch_lds(int n, const NoisyGradArgs& g, hipStream_t st) {
    switch (n) {
        case 10: return launch_lds_n<10>(g, st);
        case 11: return launch_lds_n<11>(g, st);
        case 12: return launch_lds_n<12>(g, st);
        default: return QHEA_EUNSUPPORTED;
    }
}
constexpr GradUnit kLdsUnit{10, 12, kLdsGradTile, launch_lds};

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_noisy_lds_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise) {
    return wide_grad_workspace_bytes(kLdsUnit, desc, batch, noise);
}

int qhea_model_loss_grad_noisy_lds(const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch,
                                   const double* trunk, const double* y, const double* params, const double* ham_diag,
                                   const qhea_noise* noise, double inv_batch_total, double* grad, double* pred, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    return wide_grad_loss_grad(kLdsUnit, desc, row0, batch, branch, trunk, y, params, ham_diag, noise, inv_batch_total, grad, pred,
                               workspace, workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_lds(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                     const double* branch, const double* trunk, const double* y, double* params,
                                     const double* ham_diag, const qhea_noise* noise, const double* inv_batch_total,
                                     double* grad, int64_t grad_stride, double* exp_avg, double* exp_avg_sq,
                                     int64_t first_step, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, void* workspace, size_t workspace_bytes, void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return wide_grad_train_steps(kLdsUnit, desc, call, ham_diag, noise, lr);
}

}  // extern "C"
