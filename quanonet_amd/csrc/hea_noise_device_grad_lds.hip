// hea_noise_device_grad_lds.hip -- qhea_model_loss_grad_noisy_device_lds / qhea_model_train_steps_noisy_device_lds: the MSE loss
// of the quantum-jump estimate under the calibrated device noise model and the unbiased gradient of hea_noise_device_grad.hip,
// for n = 10..12, where psi and lambda live in LDS.  Same quantity, estimator (d num_k / N2_k with the fired pattern held fixed;
// neither the norm nor the decisions are differentiated), random stream and record form (include/quanonet_hea.h); what differs is
// where the states live and, with it, the order of the sums.  tests/device_traj_grad_reference.py restates the walk in numpy.
//
// device_grad_lds_kernel<N>: a workgroup of 2^(n-4) threads walks (row, tile of kLdsDevGradTile trajectories) items in a
// grid-stride loop; psi and lambda rest in LDS in the layout LCfg<N, 4> behind the forward's scratch -- ONE pass width, 4 gate
// qubits per pass, at every n and in both directions, because relax_site's diagonal step is written for the 16 amplitudes of
// that width (64 / 128 / 256 threads at n = 10 / 11 / 12; at n = 12 2 x 64 KB of the CU's 160 KB + 2.5 KB).  Per trajectory:
//   forward   device_traj_lds_kernel's walk, the same code (segment_draws, jump_layer, relax_site of hea_noise_jump_lds.hpp): the
//             same Philox calls, words, thresholds, masked sums and u N2 < gamma M rule.  At every block's start psi~ goes into
//             the workgroup's snapshot area (each thread its own 16 LDS slots), and behind every segment thread 0 writes the
//             segment's eight words into the workgroup's record in global memory: the sites that fired (bits 0..35 of two words;
//             bit 31 of the second: the 2^100 rescale fired), the frame's X bit on the site's wire when the site was reached
//             (two words), and the frame the last store applied (phys(x), and z pulled back through the ring).  Global memory,
//             not LDS: the count of segments is the model's, not bounded by what LDS is left.  Nothing is decided or drawn twice.
//   read-out  behind the basis change thread t holds the basis states 16 t .. 16 t + 15: num and N2 in the forward kernel's
//             order, lambda = h' psi~ / N2, both back through the basis change's dagger;
//   reverse   per segment, last to first, on psi and lambda together.  The first gather is load_framed with the RECORDED frame
//             (the ring's inverse with it) and undoes the rescale (psi 2^-100, lambda 2^100).  load_framed is the exact inverse
//             of store_framed -- the store drops the frame's sign (-1)^parity(x & z) and so does every re-walk, which stores
//             through the same function -- so, unlike in the register layout, no sign is left over between a re-walked psi
//             and lambda.  Then the sites backwards inside the passes that hold them, diagonal on the thread's registers with
//             the forward's masks and the recorded polarity: no jump: psi by 1 / sqrt(1 - gamma), lambda by sqrt(1 - gamma);
//             jump: lambda by the projector (the X sits in the recorded frame), and psi -- the projector has no inverse -- from
//             the block's snapshot walked forward to the site with the recorded words (replay_layer: no draws, no masked sums,
//             no decisions; at most one block per fired jump).  Behind a site the inner products and the adjoint gate of its
//             wire, as bwd_layer of hea_lds.hpp.
// The reverse walk of a block is one loop over its segments with ONE copy of the re-walk in it: a segment's sites are undone
// behind workgroup-uniform guards (`cur` sites left; a pass runs when cur lies in its range), a fired site without its psi stops
// the pass, lambda's registers go back to the pass's own slots, the loop restores psi into the same slots and enters the same
// pass again with plain loads.
// Sums: a site's masked sum as the forward (thread, butterfly, waves in order).  The 3n (or n) inner products per thread go
// over the wave by lane_reduce, the waves in wave order through LDS, and thread i adds value i to the item's record in global
// memory -- the first trajectory of the tile stores, later ones read, add and store, the same thread every time.  No atomics.
// Records, fold and reduce are hea_noise_grad.hip's and hea_density_grad.hip's; the tables kernel's body is hea_noise_jump.hpp's.
// The host side of the calls (checks, workspace layout and query, call record, open, launch, the bodies of loss_grad and
// train_steps) is hea_noise_jump_grad.hpp's, shared with the wave form of this unit.  Here: the kernel and its device helpers, the
// tables kernel and the launcher, the unit record (JumpLdsUnit) and the extern "C" shells.
#include <climits>
#include <cmath>
#include <cstdint>

#include "hea_noise_jump_lds.hpp"
#include "hea_noise_jump_grad.hpp"

namespace qhea {
namespace {

// Trajectories per work item: part of the stated summation order; 2 as hea_noise_grad_lds.hip (its sweep).  The override is
// for a sweep.
#ifndef QHEA_DEVICE_GRAD_LDS_TILE
#define QHEA_DEVICE_GRAD_LDS_TILE 2
#endif
constexpr int kLdsDevGradTile = QHEA_DEVICE_GRAD_LDS_TILE;
constexpr int kAllSites = 64;               // `stop` of a whole segment

// Workgroups of a launch at most: each owns a snapshot area, so this bounds the workspace.  What 256 CUs keep resident: the LDS
// of a workgroup (33 / 66 / 131 KB) allows 4 / 2 / 1 per CU; more items than this go round the grid-stride loop.
constexpr int lds_grad_max_groups(int n) { return n == 10 ? 1024 : n == 11 ? 512 : n == 12 ? 256 : 0; }

// the forward's table and, beside a site's (gamma, sqrt(1 - gamma)), 1 / sqrt(1 - gamma) for the way back.  Beside, not inside:
// jump_tables_body copies a table of at most 256 words.
struct LdsDevGradTable { WideDevTable t; double inv[4][kWideWires]; };

struct LdsDevGradArgs {
    const LdsDevGradTable* tab;
    double2* snap;                          // [groups][blocks][2^n]: the LDS image of psi~ at every block's start
    unsigned* words;                        // [groups][segments][kSegWords]
    long snap_stride, words_stride;         // per workgroup, in elements
};

// ---- device helpers -------------------------------------------------------------------------------------------------------------------

struct SegRecord : SegWords {               // jump_layer's recorder
    template <int IDX>
    __device__ __forceinline__ void site(int xq, int f) {
        pol |= (unsigned long long)(unsigned)xq << IDX;
        fired |= (unsigned long long)(unsigned)f << IDX;
    }
    __device__ __forceinline__ void tail(int px_, int z_, bool r) { px = px_; z = z_; rescaled = r; }
};

__device__ __forceinline__ void store_words(unsigned* w, int seg, const SegWords& v) {
    unsigned* p = w + (long)seg * kSegWords;
    unsigned packed[6];
    pack_words(v, packed);
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = packed[i];
}
// Thread 0 wrote them, every thread reads them, a workgroup barrier in between.  The offset behind a vector-register fence: the
// loads are vector loads, which see the workgroup's own stores (a scalar load reads through another cache).
__device__ __forceinline__ SegWords load_words(const unsigned* w, int seg) {
    int lz = 0;
    asm volatile("" : "+v"(lz));
    const unsigned* p = w + (long)seg * kSegWords + lz;
    unsigned packed[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) packed[i] = (unsigned)uniform((int)p[i]);
    return unpack_words(packed);
}

// f(J, one) over the thread's 16 amplitudes: `one` = the wire whose |1> is the parity of the stored bits MASK reads |1> under
// the frame's X bit xq (relax_site's predicate)
template <int A, int MASK, class F>
__device__ __forceinline__ void for_wire(int tp, int xq, F&& f) {
    static_for<0, (1 << kLG)>([&](auto jj) { f(jj, wire_reads_one<A, MASK>(tp, xq, decltype(jj)::value)); });
}

// The thread's LDS bases behind a vector-register fence.  The 16 slot addresses of a pass are base ^ constant, which no
// immediate offset expresses, so unfenced they are loop invariants: the compiler keeps the addresses of every pass of every
// layer (forward, reverse, re-walk; psi and lambda) in registers across the whole walk, and n = 12 spills.  Behind the fence a
// layer recomputes its own (16 XORs per pass).
template <int N>
__device__ __forceinline__ Bases<N, kLG> fenced(const Bases<N, kLG>& bs) {
    Bases<N, kLG> f = bs;
#pragma unroll
    for (int p = 0; p < LCfg<N, kLG>::NP; ++p) asm volatile("" : "+v"(f.plain[p]));
    asm volatile("" : "+v"(f.ring));
    return f;
}

template <int M>
__device__ __forceinline__ void scale_all(c2 (&v)[M], double f) {
#pragma unroll
    for (int j = 0; j < M; ++j) { v[j].x *= f; v[j].y *= f; }
}

// Re-walk: site IDX from the recorded words; sites from `stop` on are left out
template <int A, int IDX, int MASK>
__device__ __forceinline__ void replay_site(c2 (&v)[1 << kLG], int tp, double2 gs, const SegWords& w, int stop) {
    if (IDX < stop && gs.x > 0.0) {
        const int xq = (int)((w.pol >> IDX) & 1ull);
        if ((w.fired >> IDX) & 1ull) {
            for_wire<A, MASK>(tp, xq, [&](auto jj, bool one) {
                constexpr int J = decltype(jj)::value;
                v[J].x = one ? v[J].x : 0.0; v[J].y = one ? v[J].y : 0.0;
            });
        } else {
            for_wire<A, MASK>(tp, xq, [&](auto jj, bool one) {
                constexpr int J = decltype(jj)::value;
                const double f = one ? gs.y : 1.0;
                v[J].x *= f; v[J].y *= f;
            });
        }
    }
}

// One gate layer of the re-walk: the gates whose site is <= stop and the sites < stop of passes 0 .., stored plain to the slots
// of the pass that holds site `stop`; a whole segment (stop == kAllSites) ends with the rescale and the recorded frame's store.
template <int N, int SITE, class G>
__device__ __forceinline__ void replay_layer(double2* s, const Bases<N, kLG>& bs, int t, const WideDevTable* __restrict__ tab,
                                             const SegWords& w, int stop, G gate) {
    constexpr int LG = kLG, NP = LCfg<N, LG>::NP;
    constexpr bool RING = SITE == kRot;
    static_for<0, NP>([&](auto p) {
        constexpr int P = decltype(p)::value;
        using PS = Pass<N, P, LG>;
        if (stop >= PS::Q0) {                                            // workgroup-uniform
            const int tp = thread_part<PS::A, LG>(t);
            c2 v[1 << LG];
            load_group<N, PS::A, false, LG>(s, bs.plain[P], v);
            static_for<PS::Q0, PS::Q1>([&](auto q) {
                constexpr int Q = decltype(q)::value;
                if (Q <= stop) apply_group<Q - PS::A, LG>(v, gate(Q));
                replay_site<PS::A, Q, (1 << Q)>(v, tp, site_pair(tab, SITE, Q), w, stop);
            });
            if constexpr (P == NP - 1) {
                if constexpr (RING) {
                    static_for<0, N>([&](auto jj) {
                        constexpr int J = decltype(jj)::value, CQ = (J + 1) % N, TQ = J;
                        replay_site<PS::A, N + 2 * J, ring_site_mask<N, J, true>()>(v, tp, site_pair(tab, kTgt, TQ), w, stop);
                        replay_site<PS::A, N + 2 * J + 1, ring_site_mask<N, J, false>()>(v, tp, site_pair(tab, kCtl, CQ), w, stop);
                    });
                }
                if (stop == kAllSites) {
                    if (w.rescaled) scale_all(v, 0x1p100);
                    __syncthreads();                       // every thread holds its amplitudes: safe to permute
                    store_framed<N, PS::A, RING, LG>(s, RING ? bs.ring : bs.plain[P], w.px, w.z, tp, v);
                } else {
                    store_group<N, PS::A, false, LG>(s, bs.plain[P], v);
                }
            } else {
                store_group<N, PS::A, false, LG>(s, bs.plain[P], v);
            }
            __syncthreads();
        }
    });
}

// Reverse: site IDX (wire W, stored-bit mask MASK, table row SITE) is undone when it is the next one (`cur` == IDX + 1) and the
// pass has not stopped.  A fired site needs psi from before the jump (`have`); without it the pass stops there.  `gate` undoes
// what the forward walk applies in front of the site.
template <int A, int IDX, int W, int MASK, int SITE, class Gate>
__device__ __forceinline__ void undo_site(c2 (&pv)[1 << kLG], c2 (&lv)[1 << kLG], int tp, const LdsDevGradTable* __restrict__ gt,
                                          const SegWords& w, int& cur, bool& have, bool& stopped, Gate&& gate) {
    if (!stopped && cur == IDX + 1) {
        const bool f = (w.fired >> IDX) & 1ull;
        if (f && !have) {
            stopped = true;
        } else {
            const double2 gs = site_pair(&gt->t, SITE, W);
            if (gs.x > 0.0) {
                const int xq = (int)((w.pol >> IDX) & 1ull);
                if (f) {                                                 // psi: already the state before the jump
                    for_wire<A, MASK>(tp, xq, [&](auto jj, bool one) {
                        constexpr int J = decltype(jj)::value;
                        lv[J].x = one ? lv[J].x : 0.0; lv[J].y = one ? lv[J].y : 0.0;
                    });
                } else {
                    const double inv = site_inv(gt, SITE, W);
                    for_wire<A, MASK>(tp, xq, [&](auto jj, bool one) {
                        constexpr int J = decltype(jj)::value;
                        const double fp = one ? inv : 1.0, fl = one ? gs.y : 1.0;
                        pv[J].x *= fp; pv[J].y *= fp;
                        lv[J].x *= fl; lv[J].y *= fl;
                    });
                }
            }
            have = false; cur = IDX;
            gate();
        }
    }
}

// One reverse layer with its sites, from site `cur` down; see the head of the file.  `fresh`: the segment is entered from
// behind, so its first gather is the framed one.  gate(q) returns the ADJOINT coefficients of wire q's gate; acc: a sub-layer's
// [3q .. 3q + 2], an encoding layer's [q].
template <int N, int SITE, class G, int NA>
__device__ __forceinline__ void undo_layer(double2* psi, double2* lam, const Bases<N, kLG>& bs, int t,
                                           const LdsDevGradTable* __restrict__ gt, const SegWords& w, int& cur, bool& have,
                                           bool& stopped, bool& fresh, double (&acc)[NA], G gate) {
    constexpr int LG = kLG, NP = LCfg<N, LG>::NP, M = 1 << LG;
    constexpr bool RING = SITE == kRot;
    static_rfor<0, NP>([&](auto p) {
        constexpr int P = decltype(p)::value;
        using PS = Pass<N, P, LG>;
        if (!stopped && cur > PS::Q0) {                                  // workgroup-uniform
            const int tp = thread_part<PS::A, LG>(t);
            c2 pv[M], lv[M];
            if (P == NP - 1 && fresh) {
                load_framed<N, PS::A, RING, LG>(psi, RING ? bs.ring : bs.plain[P], w.px, w.z, tp, pv);
                load_framed<N, PS::A, RING, LG>(lam, RING ? bs.ring : bs.plain[P], w.px, w.z, tp, lv);
                __syncthreads();                           // all gathers done before anything is overwritten
                if (w.rescaled) { scale_all(pv, 0x1p-100); scale_all(lv, 0x1p100); }
                fresh = false;
            } else {
                load_group<N, PS::A, false, LG>(psi, bs.plain[P], pv);
                load_group<N, PS::A, false, LG>(lam, bs.plain[P], lv);
            }
            if constexpr (RING && P == NP - 1) {
                static_rfor<0, N>([&](auto jj) {
                    constexpr int J = decltype(jj)::value, CQ = (J + 1) % N, TQ = J;
                    undo_site<PS::A, N + 2 * J + 1, CQ, ring_site_mask<N, J, false>(), kCtl>(pv, lv, tp, gt, w, cur, have, stopped,
                                                                                            [] {});
                    undo_site<PS::A, N + 2 * J, TQ, ring_site_mask<N, J, true>(), kTgt>(pv, lv, tp, gt, w, cur, have, stopped, [] {});
                });
            }
            static_rfor<PS::Q0, PS::Q1>([&](auto q) {
                constexpr int Q = decltype(q)::value;
                constexpr int LBIT = Q - PS::A;
                undo_site<PS::A, Q, Q, (1 << Q), SITE>(pv, lv, tp, gt, w, cur, have, stopped, [&] {
                    const double4 u = gate(Q);
                    static_for<0, M>([&](auto jj) {
                        constexpr int J = decltype(jj)::value;
                        if constexpr (!(J & (1 << LBIT))) {
                            constexpr int J1 = J | (1 << LBIT);
                            if constexpr (RING) inner(pv[J], pv[J1], lv[J], lv[J1], acc[3 * Q], acc[3 * Q + 1], acc[3 * Q + 2]);
                            else inner_x(pv[J], pv[J1], lv[J], lv[J1], acc[Q]);
                            su2(pv[J], pv[J1], u);
                            su2(lv[J], lv[J1], u);
                        }
                    });
                });
            });
            store_group<N, PS::A, false, LG>(lam, bs.plain[P], lv);
            if (!stopped) {
                store_group<N, PS::A, false, LG>(psi, bs.plain[P], pv);
                // the next pass: P - 1, or the last pass of the following (earlier) layer
                pass_sync<(P > 0) && wave_local_passes<N, LG, P, (P > 0 ? P - 1 : 0)>()>();
            }
        }
    });
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------

template <int N>
__global__ __launch_bounds__((LCfg<N, kLG>::T)) void device_grad_lds_kernel(NoisyGradArgs g, LdsDevGradArgs d) {
    constexpr int LG = kLG, M = 1 << LG;
    using L = LCfg<N, LG>;
    constexpr int KW = L::KW;
    extern __shared__ __attribute__((aligned(16))) char grad_lds[];
    JumpScratch* sc = reinterpret_cast<JumpScratch*>(grad_lds);
    double2* psi = reinterpret_cast<double2*>(grad_lds + kScratchBytes);
    double2* lam = psi + L::DIM;
    double* red = reinterpret_cast<double*>(lam + L::DIM);               // [NW][64]: per-wave sums of the inner products
    const NoiseArgs& a = g.f;
    const LdsDevGradTable* __restrict__ gt = d.tab;
    const WideDevTable* __restrict__ tab = &d.tab->t;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double2* snap = d.snap + (long)blockIdx.x * d.snap_stride;           // block b: snap[b * 2^n + LDS slot]
    unsigned* words = d.words + (long)blockIdx.x * d.words_stride;
    Bases<N, LG> bs;
    bs.init(t);
    const double off_term = a.diag ? 0.0 : a.off;
    constexpr double kR = 0.70710678118654752440;
    const long items = a.B * a.tiles;

    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long r = item / a.tiles, t0 = (item - r * a.tiles) * (long)kLdsDevGradTile;
        const int tcount = (int)(a.T - t0 < kLdsDevGradTile ? a.T - t0 : kLdsDevGradTile);
        const unsigned long long row = (unsigned long long)(a.row0 + r);
        const double2* csr = a.cs + r * a.E;
        double* rec = g.items + item * (long)g.width;
        double* rec_w = rec + a.E;

        double sum = 0.0, sq = 0.0;
        for (int tj = 0; tj < tcount; ++tj) {
            const unsigned traj = (unsigned)(t0 + tj);
            const bool first = tj == 0;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const int p = t + j * L::T;
                psi[p] = make_double2(p == 0 ? 1.0 : 0.0, 0.0);          // |0..0>: phys(0) = 0
            }
            JumpState js{1.0, 0, 0, 0};
            unsigned call = 0;
            int s = 0, col = 0, seg = 0, blk = 0;
            // ---- forward: device_traj_lds_kernel's walk, with the snapshots and the segments' words
            for (int gi = 0; gi < 2; ++gi) {
                for (int b = 0; b < a.nb[gi]; ++b, ++blk) {
#pragma unroll
                    for (int j = 0; j < M; ++j) {                        // the slots this thread filled or a barrier covers
                        const int p = t + j * L::T;
                        snap[(long)blk * L::DIM + p] = psi[p];
                    }
                    segment_draws(a, tab, sc, call, 0, N, N, traj, row); // its barrier also covers the initial state
                    SegRecord rc{};
                    jump_layer<N, kEnc>(psi, fenced<N>(bs), t, sc, tab, js, [&](int q) { return rx_su2(csr[col + q]); }, rc);
                    if (t == 0) store_words(words, seg, rc);
                    ++seg; col += N; call += N;
                    for (int l = 0; l < a.ld[gi]; ++l, ++s, ++seg) {
                        segment_draws(a, tab, sc, call, N, 3 * N, N, traj, row);
                        SegRecord rs{};
                        jump_layer<N, kRot>(psi, fenced<N>(bs), t, sc, tab, js, [&](int q) { return a.gates[2 * ((s + 1) * N + q)]; }, rs);
                        if (t == 0) store_words(words, seg, rs);
                        call += 3 * N;
                    }
                }
            }
            // ---- read-out: the forward kernel's value; lambda = h' psi~ / N2
            if (a.pauli != QHEA_PAULI_Z) {                               // same probabilities as H / H S^dagger
                const double4 ub = a.pauli == QHEA_PAULI_X ? make_double4(kR, 0.0, kR, 0.0) : make_double4(kR, 0.0, 0.0, -kR);
                plain_layer<N>(psi, fenced<N>(bs), [&](int) { return ub; });
            }
            {
                // thread t reads the 16 consecutive basis states 16 t .. 16 t + 15
                c2 v[M], lv[M];
                load_group<N, 0, false, LG>(psi, bs.plain[0], v);
                double part = 0.0, num = 0.0;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const double pk = v[j].x * v[j].x + v[j].y * v[j].y;
                    part += pk;
                    num += pk * g.hd[(t << LG) | j];
                }
                num = group_sum<6>(num);
                double tot = group_sum<6>(part);
                if constexpr (L::NW > 1) {
                    if (lane == 0) { sc->rsum[0][wave] = num; sc->rsum[1][wave] = tot; }
                    __syncthreads();
                    num = sc->rsum[0][0]; tot = sc->rsum[1][0];
#pragma unroll
                    for (int w = 1; w < L::NW; ++w) { num += sc->rsum[0][w]; tot += sc->rsum[1][w]; }
                }
                const double val = num / tot + off_term;
                sum += val; sq += val * val;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const double hk = g.hd[(t << LG) | j];
                    lv[j].x = hk * v[j].x / tot; lv[j].y = hk * v[j].y / tot;
                }
                store_group<N, 0, false, LG>(lam, bs.plain[0], lv);
                __syncthreads();                                         // lambda is whole; rsum is free again
            }
            if (a.pauli != QHEA_PAULI_Z) {
                const double4 ud = a.pauli == QHEA_PAULI_X ? make_double4(kR, 0.0, -kR, 0.0) : make_double4(kR, 0.0, 0.0, kR);
                plain_layer<N>(psi, fenced<N>(bs), [&](int) { return ud; });
                plain_layer<N>(lam, fenced<N>(bs), [&](int) { return ud; });
            }
            // ---- reverse: blocks backwards; per block one loop over its segments (l = ld .. 1 sub-layers, 0 the encoding)
            for (int gi = 1; gi >= 0; --gi) {
                const int ldg = a.ld[gi];
                for (int b = a.nb[gi] - 1; b >= 0; --b) {
                    --blk; s -= ldg; col -= N; seg -= 1 + ldg;           // the block's first sub-layer, columns and segment
                    int l = ldg, cur = 0;
                    bool enter = true, have = false, fresh = false;
                    SegWords w{};
                    double acc[3 * N];                                  // not KW: live across the re-walk
                    for (;;) {
                        if (enter) {
                            w = load_words(words, seg + l);
                            cur = l ? 3 * N : N;
                            have = false; enter = false; fresh = true;
#pragma unroll
                            for (int i = 0; i < 3 * N; ++i) acc[i] = 0.0;
                        }
                        bool stopped = false;
                        if (l) {
                            const int sl = s + l - 1;
                            undo_layer<N, kRot>(psi, lam, fenced<N>(bs), t, gt, w, cur, have, stopped, fresh, acc,
                                                [&](int q) { return dagger(a.gates[2 * ((sl + 1) * N + q)]); });
                        } else {
                            undo_layer<N, kEnc>(psi, lam, fenced<N>(bs), t, gt, w, cur, have, stopped, fresh, acc,
                                                [&](int q) { return dagger(rx_su2(csr[col + q])); });
                        }
                        if (cur == 0) {                                  // the segment is done: its sums into the item's record
                            if (l) {
                                double xyz[KW];
#pragma unroll
                                for (int i = 0; i < KW; ++i) xyz[i] = i < 3 * N ? acc[i] : 0.0;
                                lane_reduce<KW, 6>(xyz, lane);           // lane i holds the wave total of value i
                                if (lane < KW) red[wave * 64 + lane] = xyz[0];
                                __syncthreads();
                                if (t < 3 * N) {
                                    double tot = red[t];
#pragma unroll
                                    for (int wv = 1; wv < L::NW; ++wv) tot += red[wv * 64 + t];
                                    double* p = rec_w + (long)(s + l - 1) * 3 * N + t;
                                    *p = first ? tot : *p + tot;
                                }
                                --l; enter = true;
                                continue;
                            }
                            double gx[16];
#pragma unroll
                            for (int i = 0; i < 16; ++i) gx[i] = i < N ? acc[i] : 0.0;
                            lane_reduce<16, 6>(gx, lane);                // lane j holds the wave total of value j & 15
                            if (lane < 16) red[wave * 64 + lane] = gx[0];
                            __syncthreads();
                            if (t < N) {
                                double tot = red[t];
#pragma unroll
                                for (int wv = 1; wv < L::NW; ++wv) tot += red[wv * 64 + t];
                                double* p = rec + col + t;
                                *p = first ? tot : *p + tot;
                            }
                            break;
                        }
                        // a fired site: psi from before the jump -- the block's snapshot walked forward to site cur - 1.  The
                        // barrier: every wave has its registers of the stopped pass before psi is overwritten
                        // (QHEA_DEVICE_GRAD_SKIP_REWALK: timing builds only, wrong results -- the share of the re-walks)
                        __syncthreads();
#ifndef QHEA_DEVICE_GRAD_SKIP_REWALK
#pragma unroll
                        for (int j = 0; j < M; ++j) {
                            const int p = t + j * L::T;
                            psi[p] = snap[(long)blk * L::DIM + p];
                        }
                        __syncthreads();
                        replay_layer<N, kEnc>(psi, fenced<N>(bs), t, tab, load_words(words, seg), l ? kAllSites : cur - 1,
                                              [&](int q) { return rx_su2(csr[col + q]); });
                        for (int j = 1; j <= l; ++j) {
                            const int sj = s + j - 1;
                            replay_layer<N, kRot>(psi, fenced<N>(bs), t, tab, load_words(words, seg + j), j == l ? cur - 1 : kAllSites,
                                                  [&](int q) { return a.gates[2 * ((sj + 1) * N + q)]; });
                        }
#endif
                        have = true;
                    }
                }
            }
            __syncthreads();                                             // psi, the scratch and `red` are rewritten
        }
        if (t == 0) a.partial[item] = make_double2(sum, sq);
    }
}

__global__ __launch_bounds__(256) void device_grad_lds_tables_kernel(LdsDevGradTable t, LdsDevGradTable* __restrict__ out,
                                                                     const double* __restrict__ diag, double co, int n,
                                                                     double* __restrict__ buf) {
    if (threadIdx.x < 4 * kWideWires) (&out->inv[0][0])[threadIdx.x] = (&t.inv[0][0])[threadIdx.x];
    jump_tables_body(t.t, &out->t, diag, co, n, buf);
}

template <int N>
int launch_device_grad_lds_n(const NoisyGradArgs& g, const LdsDevGradArgs& d, int groups, hipStream_t st) {
    using L = LCfg<N, kLG>;
    constexpr size_t smem = kScratchBytes + 2 * L::STATE_BYTES + (size_t)L::NW * 64 * sizeof(double);
    return launch_dynamic_lds(device_grad_lds_kernel<N>, dim3((unsigned)groups), dim3(L::T), smem, st, g, d);
}
int launch_device_grad_lds(int n, const NoisyGradArgs& g, const LdsDevGradArgs& d, int groups, hipStream_t st) {
    switch (n) {
        case 10: return launch_device_grad_lds_n<10>(g, d, groups, st);
        case 11: return launch_device_grad_lds_n<11>(g, d, groups, st);
        case 12: return launch_device_grad_lds_n<12>(g, d, groups, st);
        default: return QHEA_EUNSUPPORTED;
    }
}

// ---- the unit of hea_noise_jump_grad.hpp's host body ------------------------------------------------------------------------------------

struct JumpLdsUnit {
    using Table = LdsDevGradTable;
    using Args = LdsDevGradArgs;
    using Snap = double2;
    static constexpr GradUnit unit{10, 12, kLdsDevGradTile, nullptr};    // the layout's qubit range and tile
    static WideDevTable& jump(Table& t) { return t.t; }
    static const WideDevTable& jump(const Table& t) { return t.t; }
    static constexpr int cap(int n) { return lds_grad_max_groups(n); }
    static long words_stride(long segs) { return segs * kSegWords; }
    static long snap_stride(long blocks, int n) { return blocks << n; }  // double2 per LDS slot and block
    static void launch_tables(const Table& tb, Table* out, const double* diag, double co, int n, double* buf, hipStream_t st) {
        hipLaunchKernelGGL(device_grad_lds_tables_kernel, dim3(1), dim3(256), 0, st, tb, out, diag, co, n, buf);
    }
    static int launch(int n, const NoisyGradArgs& g, const Args& d, int groups, hipStream_t st) {
        return launch_device_grad_lds(n, g, d, groups, st);
    }
};

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

int qhea_noisy_device_lds_grad_max_workgroups(int n) { return lds_grad_max_groups(n); }

size_t qhea_model_noisy_device_lds_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling) {
    return jump_grad_workspace_bytes<JumpLdsUnit>(desc, batch, sampling);
}

int qhea_model_loss_grad_noisy_device_lds(const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch,
                                          const double* trunk, const double* y, const double* params, const double* ham_diag,
                                          const qhea_device_noise* dn, const qhea_sampling* sampling, double inv_batch_total,
                                          double* grad, double* pred, void* workspace, size_t workspace_bytes, void* stream) {
    return jump_grad_loss_grad<JumpLdsUnit>(desc, row0, batch, branch, trunk, y, params, ham_diag, dn, sampling, inv_batch_total,
                                            grad, pred, workspace, workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_device_lds(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                            const double* branch, const double* trunk, const double* y, double* params,
                                            const double* ham_diag, const qhea_device_noise* dn, const qhea_sampling* sampling,
                                            const double* inv_batch_total, double* grad, int64_t grad_stride, double* exp_avg,
                                            double* exp_avg_sq, int64_t first_step, double lr, double beta1, double beta2,
                                            double eps, double weight_decay, void* workspace, size_t workspace_bytes, void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return jump_grad_train_steps<JumpLdsUnit>(desc, call, ham_diag, dn, sampling, lr);
}

}  // extern "C"
