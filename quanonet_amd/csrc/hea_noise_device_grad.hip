// hea_noise_device_grad.hip -- qhea_model_loss_grad_noisy_device / qhea_model_train_steps_noisy_device: the MSE loss of the
// quantum-jump estimate under the calibrated device noise model (hea_noise_device.hip, expectation mode) and an unbiased
// gradient of it, n = 7..9.  The contract is stated in include/quanonet_hea.h; tests/device_traj_grad_reference.py restates the
// walk in numpy.
//
// The estimator.  With the fired pattern k of a trajectory held fixed, its unnormalised final state psi~_k is the product of
// fixed linear operators (gates, sampled Paulis, K0 = diag(1, sqrt(1 - gamma)) where no jump fired, L = |0><1| where one did).
// The pattern's probability is c_k N2_k with N2_k = <psi~_k|psi~_k> and c_k free of the parameters, the trajectory's value is
// num_k / N2_k with num_k = <psi~_k|h'|psi~_k>, so the exact value is sum_k c_k num_k and its derivative is
// E_k[ d num_k / N2_k ]: the gradient of the unnormalised numerator with the pattern fixed, divided by the final N2.  The norm
// and the jump decisions are NOT differentiated (their two terms cancel).
//
// device_grad_wave_kernel<N>: a wave walks (row, tile of kDevGradTile trajectories) items in a grid-stride loop, the state in
// Cfg<N>'s layout.  Per trajectory:
//   forward   device_traj_wave_kernel's walk (the same Philox calls, words, thresholds, masked sums and u nrm2 < gamma M rule);
//             at every block's start psi~ goes into the wave's snapshot area, and behind every segment four words go into its
//             record: the sites that fired (bit 31: the 2^100 rescale fired), the polarity of the frame at every site, and the
//             segment's final frame (X mask, Z mask).  The reverse walk and the re-walks read them: nothing is decided or drawn
//             twice;
//   read-out  lambda = h' psi~ / N2 behind basis_change, both back through its dagger;
//   reverse   per segment: the rescale (psi 2^-100, lambda 2^100: psi stays in the scale the forward walk had there, which is
//             the snapshots'), the frame on both with its sign (-1)^parity(x & z), then the sites backwards.  No jump: psi by
//             K0^-1, lambda by K0.  Jump: lambda by L^dagger (with the site's polarity), and psi -- L has no inverse -- from
//             the block's snapshot walked forward to the site with the recorded words (at most one block per fired jump).
//             The gates as in noisy_grad_wave_kernel.
// The reverse walk of a block is one loop over its segments with ONE copy of the re-walk in it: a segment's sites are undone
// behind wave-uniform guards (`cur` sites left), a fired site without its psi stops the pass, the loop restores psi and enters
// the same segment again.
// Records, fold and reduce are hea_noise_grad.hip's and hea_density_grad.hip's, unchanged; the tables kernel's body is
// hea_noise_jump.hpp's.  The forward pieces below (site_draws, the relaxation of a site, the rescale) restate
// hea_noise_device.hip's, which keeps its own text: its device code is pinned (profiles/r31_device_code_identity.txt).
// The fenced read of 1 / sqrt(1 - gamma) and the host side of the calls (checks, workspace layout and query, call record, open,
// launch, the bodies of loss_grad and train_steps) are hea_noise_jump_grad.hpp's, shared with the LDS form of this unit
// (hea_noise_device_grad_lds.hip, n = 10..12).  Here: the kernels and their device helpers, the tables kernel and the launcher,
// the unit record (JumpWaveUnit) and the extern "C" shells.
#include <climits>
#include <cmath>
#include <cstdint>

#include "hea_noise_jump_grad.hpp"

namespace qhea {
namespace {

constexpr int kDevGradWaves = 4;            // waves per workgroup (independent; no LDS, no barrier)
#ifndef QHEA_DEVICE_GRAD_TILE
#define QHEA_DEVICE_GRAD_TILE 4
#endif
constexpr int kDevGradTile = QHEA_DEVICE_GRAD_TILE;   // trajectories per work item: part of the stated summation order
// Waves of a launch at most: each owns a snapshot area, so this bounds the workspace.  2 waves per SIMD (what 256 VGPRs allow)
// on 256 CUs; more items than this go round the grid-stride loop.
constexpr int kDevGradMaxWaves = 2048;
constexpr int kAllSites = 64;               // `stop` of a whole segment
static_assert(kDevGradMaxWaves % kDevGradWaves == 0, "whole workgroups");

// the forward's table and, beside a site's (gamma, sqrt(1 - gamma)), 1 / sqrt(1 - gamma) for the way back
struct DevGradTable : JumpTable<kJumpMaxWires> { double inv[4][kJumpMaxWires]; };

struct DevGradArgs {
    const DevGradTable* tab;
    double* snap;                           // [waves][blocks][2 R][64]: psi~ at every block's start
    unsigned* words;                        // [waves][segments][4][64]: fired | rescale << 31, polarity, frame X, frame Z
    long snap_stride, words_stride;         // per wave, in elements
    int waves;
};

// ---- device helpers -------------------------------------------------------------------------------------------------------------------

template <bool RING>
__device__ __forceinline__ void site_draws(const NoiseArgs& a, const DevGradTable* __restrict__ tab, unsigned call0, int tbase,
                                           int cnt, int c, unsigned traj, unsigned long long row, unsigned& code, unsigned& w3) {
    code = 0; w3 = 0;
    if (a.thr1 == 0 || c >= cnt) return;
    const uint4 w = philox(make_uint4(call0 + (unsigned)c, traj, (unsigned)row, (unsigned)(row >> 32)), a.key0, a.key1);
    draw_code(tab, tbase + c, w, (RING && !(c & 1)) ? 15u : 3u, code, w3);
}

__device__ __forceinline__ unsigned lane_word(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane((int)v, l); }

// amplitude lane | r << 6 has wire Q stored as |1> under the frame's X bit xq
template <int N, int Q>
__device__ __forceinline__ bool wire_one(int lane, int r, int xq) {
    using C = Cfg<N>;
    return ((Q < C::LB ? (lane >> Q) : (r >> (Q >= C::LB ? Q - C::LB : 0))) & 1) != xq;
}

// the fired jump on the stored state: the |1> half moves to the |0> half, the |1> half is cleared
template <int N, int Q>
__device__ __forceinline__ void jump_lower(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], int xq, int lane) {
    using C = Cfg<N>;
    constexpr int R = C::R;
    if constexpr (Q < C::LB) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool one = wire_one<N, Q>(lane, r, xq);
            const double pr = xchg<(1 << Q)>(re[r]), pi = xchg<(1 << Q)>(im[r]);
            re[r] = one ? 0.0 : pr; im[r] = one ? 0.0 : pi;
        }
    } else {
        constexpr int J = 1 << (Q - C::LB);
#pragma unroll
        for (int r0 = 0; r0 < R; ++r0) {
            if (r0 & J) continue;
            const int r1 = r0 | J;
            const double lr = xq ? 0.0 : re[r1], li = xq ? 0.0 : im[r1];
            const double hr = xq ? re[r0] : 0.0, hi = xq ? im[r0] : 0.0;
            re[r0] = lr; im[r0] = li; re[r1] = hr; im[r1] = hi;
        }
    }
}

// its adjoint: the |0> half moves to the |1> half, the |0> half is cleared
template <int N, int Q>
__device__ __forceinline__ void jump_raise(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], int xq, int lane) {
    using C = Cfg<N>;
    constexpr int R = C::R;
    if constexpr (Q < C::LB) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool one = wire_one<N, Q>(lane, r, xq);
            const double pr = xchg<(1 << Q)>(re[r]), pi = xchg<(1 << Q)>(im[r]);
            re[r] = one ? pr : 0.0; im[r] = one ? pi : 0.0;
        }
    } else {
        constexpr int J = 1 << (Q - C::LB);
#pragma unroll
        for (int r0 = 0; r0 < R; ++r0) {
            if (r0 & J) continue;
            const int r1 = r0 | J;
            const double lr = xq ? re[r1] : 0.0, li = xq ? im[r1] : 0.0;
            const double hr = xq ? 0.0 : re[r0], hi = xq ? 0.0 : im[r0];
            re[r0] = lr; im[r0] = li; re[r1] = hr; im[r1] = hi;
        }
    }
}

// the |1> half of wire Q times f
template <int N, int Q>
__device__ __forceinline__ void scale_one(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], int xq, double f, int lane) {
#pragma unroll
    for (int r = 0; r < Cfg<N>::R; ++r) {
        const double m = wire_one<N, Q>(lane, r, xq) ? f : 1.0;
        re[r] *= m; im[r] *= m;
    }
}

// Forward: dephasing and damping of site IDX of its segment on wire Q, as relax_regs of hea_noise_device.hip decides it; the
// site's polarity and whether it fired go into the segment's words.
template <int N, int Q, int IDX>
__device__ __forceinline__ void relax_decide(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], double& nrm2, int x, int& z,
                                             unsigned c, unsigned w3, double2 gs, int lane, unsigned& fired, unsigned& pol) {
    using C = Cfg<N>;
    const double g = gs.x, s = gs.y;
    constexpr int R = C::R;
    z ^= (int)((c >> 4) & 1u) << Q;
    if (g > 0.0) {
        const int xq = (x >> Q) & 1;
        pol |= (unsigned)xq << IDX;
        double M = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) M += wire_one<N, Q>(lane, r, xq) ? re[r] * re[r] + im[r] * im[r] : 0.0;
        M = group_sum<6>(M);
        const bool fire = jump_u(w3) * nrm2 < g * M;                     // the same in every lane
        if (__any(fire)) {
            jump_lower<N, Q>(re, im, xq, lane);
            nrm2 = M;
            fired |= 1u << IDX;
        } else {
            scale_one<N, Q>(re, im, xq, s, lane);
            nrm2 -= g * M;
        }
    }
}

// Re-walk: the same site from the recorded words; sites from `stop` on are left out
template <int N, int Q, int IDX>
__device__ __forceinline__ void relax_replay(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], double2 gs, unsigned fired,
                                             unsigned pol, int stop, int lane) {
    if (IDX < stop && gs.x > 0.0) {
        const int xq = (int)((pol >> IDX) & 1u);
        if ((fired >> IDX) & 1u) jump_lower<N, Q>(re, im, xq, lane);
        else scale_one<N, Q>(re, im, xq, gs.y, lane);
    }
}

// Reverse: site IDX is undone when it is the next one (`cur` == IDX + 1) and the pass has not stopped.  A fired site needs psi
// from before the jump (`have`); without it the pass stops there.  `gate` undoes what the forward walk applies in front of the site.
template <int N, int Q, int IDX, int SITE, class Gate>
__device__ __forceinline__ void relax_undo(double (&pr)[Cfg<N>::R], double (&pi)[Cfg<N>::R], double (&lr)[Cfg<N>::R],
                                           double (&li)[Cfg<N>::R], const DevGradTable* __restrict__ tab, unsigned fired,
                                           unsigned pol, int& cur, bool& have, bool& stopped, int lane, Gate&& gate) {
    if (!stopped && cur == IDX + 1) {
        const bool f = (fired >> IDX) & 1u;
        if (f && !have) {
            stopped = true;
        } else {
            const double2 gs = site_pair(tab, SITE, Q);
            if (gs.x > 0.0) {
                const int xq = (int)((pol >> IDX) & 1u);
                if (f) {
                    jump_raise<N, Q>(lr, li, xq, lane);                  // psi: already the state before the jump
                } else {
                    scale_one<N, Q>(pr, pi, xq, site_inv(tab, SITE, Q), lane);
                    scale_one<N, Q>(lr, li, xq, gs.y, lane);
                }
            }
            have = false; cur = IDX;
            gate();
        }
    }
}

struct SegWords { unsigned fired, pol; int x, z; };

__device__ __forceinline__ void store_words(unsigned* w, int seg, int lane, const SegWords& v) {
    unsigned* p = w + ((long)seg * 4) * 64 + lane;                       // every lane keeps its own copy: read back by the same lane
    p[0] = v.fired; p[64] = v.pol; p[128] = (unsigned)v.x; p[192] = (unsigned)v.z;
}
__device__ __forceinline__ SegWords load_words(const unsigned* w, int seg, int lane) {
    const unsigned* p = w + ((long)seg * 4) * 64 + lane;
    return {(unsigned)uniform((int)p[0]), (unsigned)uniform((int)p[64]), uniform((int)p[128]), uniform((int)p[192])};
}

// the re-walk of an encoding segment and of a sub-layer: gates whose site is <= stop, sites < stop; a whole segment
// (stop == kAllSites) ends with its frame and rescale
template <int N>
__device__ __forceinline__ void replay_tail(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], const SegWords& v, int stop, int lane) {
    if (stop == kAllSites) {
        frame_regs<N>(re, im, v.x, v.z, lane);
        if (v.fired >> 31) {
#pragma unroll
            for (int r = 0; r < Cfg<N>::R; ++r) { re[r] *= 0x1p100; im[r] *= 0x1p100; }
        }
    }
}
template <int N>
__device__ __forceinline__ void replay_enc(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], const DevGradTable* __restrict__ tab,
                                           const double2* __restrict__ cs, const SegWords& v, int stop, int lane) {
    static_for<0, N>([&](auto q) {
        constexpr int Q = decltype(q)::value;
        if (Q <= stop) {
            const double2 c = cs[Q];
            apply_rx<N, Q>(re, im, c.x, c.y);
        }
        relax_replay<N, Q, Q>(re, im, site_pair(tab, kEnc, Q), v.fired, v.pol, stop, lane);
    });
    replay_tail<N>(re, im, v, stop, lane);
}
template <int N>
__device__ __forceinline__ void replay_sub(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], const DevGradTable* __restrict__ tab,
                                           const double4* __restrict__ gates, int s, const SegWords& v, int stop, int lane) {
    using C = Cfg<N>;
    static_for<0, N>([&](auto q) {
        constexpr int Q = decltype(q)::value;
        constexpr bool kSigned = Q < C::LB && !kSwapQubit<N, Q>;
        if (Q <= stop) {
            const double4 u = gates[2 * (s * N + Q + N) + (kSigned ? (lane >> Q) & 1 : 0)];
            apply_su2<N, Q>(re, im, u.x, u.y, u.z, u.w);
        }
        relax_replay<N, Q, Q>(re, im, site_pair(tab, kRot, Q), v.fired, v.pol, stop, lane);
    });
    static_for<0, N>([&](auto jj) {
        constexpr int J = decltype(jj)::value, CQ = (J + 1) % N, TQ = J;
        if (N + 2 * J <= stop) apply_cnot<N, CQ, TQ>(re, im, lane);
        relax_replay<N, TQ, N + 2 * J>(re, im, site_pair(tab, kTgt, TQ), v.fired, v.pol, stop, lane);
        relax_replay<N, CQ, N + 2 * J + 1>(re, im, site_pair(tab, kCtl, CQ), v.fired, v.pol, stop, lane);
    });
    replay_tail<N>(re, im, v, stop, lane);
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------

template <int N>
__global__ __launch_bounds__(64 * kDevGradWaves) void device_grad_wave_kernel(NoisyGradArgs g, DevGradArgs d) {
    using C = Cfg<N>;
    constexpr int R = C::R;
    const NoiseArgs& a = g.f;
    const DevGradTable* __restrict__ tab = d.tab;
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * kDevGradWaves + (threadIdx.x >> 6);
    if (wave >= d.waves) return;                                         // whole waves
    double* snap = d.snap + wave * d.snap_stride + lane;    // block b, register i: snap[(b * 2 R + i) * 64]
    unsigned* words = d.words + wave * d.words_stride;
    const double off_term = a.diag ? 0.0 : a.off;
    const long items = a.B * a.tiles;

    for (long item = wave; item < items; item += d.waves) {
        const long r = item / a.tiles, t0 = (item - r * a.tiles) * (long)kDevGradTile;
        const int tcount = (int)(a.T - t0 < kDevGradTile ? a.T - t0 : kDevGradTile);
        const unsigned long long row = (unsigned long long)(a.row0 + r);
        const double2* csr = a.cs + r * a.E;
        double* rec = g.items + item * (long)g.width;
        double* rec_w = rec + a.E;

        double sum = 0.0, sq = 0.0;
        for (int tj = 0; tj < tcount; ++tj) {
            const unsigned traj = (unsigned)(t0 + tj);
            const bool first = tj == 0;
            double pr[R], pi[R], lr[R], li[R], nrm2 = 1.0;
#pragma unroll
            for (int i = 0; i < R; ++i) { pr[i] = 0.0; pi[i] = 0.0; }
            pr[0] = lane == 0 ? 1.0 : 0.0;
            unsigned call = 0, code, w3;
            int s = 0, col = 0, seg = 0, blk = 0;
            // ---- forward: device_traj_wave_kernel's walk, with the snapshots and the segments' words
            for (int gi = 0; gi < 2; ++gi) {
                for (int b = 0; b < a.nb[gi]; ++b, ++blk) {
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        snap[((long)blk * 2 * R + i) * 64] = pr[i];
                        snap[((long)blk * 2 * R + R + i) * 64] = pi[i];
                    }
                    site_draws<false>(a, tab, call, 0, N, lane, traj, row, code, w3);
                    int x = 0, z = 0;
                    SegWords v{0u, 0u, 0, 0};
                    static_for<0, N>([&](auto q) {                       // encoding RX, then site ENC
                        constexpr int Q = decltype(q)::value;
                        const double2 c = csr[col + Q];
                        apply_rx<N, Q>(pr, pi, c.x, c.y);
                        const unsigned cq = lane_word(code, Q);
                        x ^= pauli_x(cq & 3u, Q); z ^= pauli_z(cq & 3u, Q);
                        relax_decide<N, Q, Q>(pr, pi, nrm2, x, z, cq, lane_word(w3, Q), site_pair(tab, kEnc, Q), lane, v.fired, v.pol);
                    });
                    frame_regs<N>(pr, pi, x, z, lane);
                    if (__any(nrm2 < 0x1p-200)) {
#pragma unroll
                        for (int i = 0; i < R; ++i) { pr[i] *= 0x1p100; pi[i] *= 0x1p100; }
                        nrm2 *= 0x1p200;
                        v.fired |= 1u << 31;
                    }
                    v.x = x; v.z = z;
                    store_words(words, seg, lane, v);
                    ++seg; col += N; call += N;
                    for (int l = 0; l < a.ld[gi]; ++l, ++s, ++seg) {
                        site_draws<false>(a, tab, call, N, N, lane, traj, row, code, w3);
                        x = 0; z = 0;
                        v = SegWords{0u, 0u, 0, 0};
                        static_for<0, N>([&](auto q) {                   // fused RY RZ RY, then site ROT
                            constexpr int Q = decltype(q)::value;
                            constexpr bool kSigned = Q < C::LB && !kSwapQubit<N, Q>;
                            const double4 u = a.gates[2 * (s * N + Q + N) + (kSigned ? (lane >> Q) & 1 : 0)];
                            apply_su2<N, Q>(pr, pi, u.x, u.y, u.z, u.w);
                            const unsigned cq = lane_word(code, Q);
                            x ^= pauli_x(cq & 3u, Q); z ^= pauli_z(cq & 3u, Q);
                            relax_decide<N, Q, Q>(pr, pi, nrm2, x, z, cq, lane_word(w3, Q), site_pair(tab, kRot, Q), lane, v.fired,
                                                  v.pol);
                        });
                        call += N;
                        site_draws<true>(a, tab, call, 2 * N, 2 * N, lane, traj, row, code, w3);
                        static_for<0, N>([&](auto jj) {                  // slot j: CNOT(c -> t), pair Pauli, TGT of t, CTL of c
                            constexpr int J = decltype(jj)::value, CQ = (J + 1) % N, TQ = J;
                            apply_cnot<N, CQ, TQ>(pr, pi, lane);
                            x ^= ((x >> CQ) & 1) << TQ;
                            z ^= ((z >> TQ) & 1) << CQ;
                            const unsigned c0 = lane_word(code, 2 * J), c1 = lane_word(code, 2 * J + 1);
                            const unsigned p = c0 & 15u;
                            x ^= pauli_x(p >> 2, CQ) | pauli_x(p & 3u, TQ);
                            z ^= pauli_z(p >> 2, CQ) | pauli_z(p & 3u, TQ);
                            relax_decide<N, TQ, N + 2 * J>(pr, pi, nrm2, x, z, c0, lane_word(w3, 2 * J), site_pair(tab, kTgt, TQ), lane,
                                                           v.fired, v.pol);
                            relax_decide<N, CQ, N + 2 * J + 1>(pr, pi, nrm2, x, z, c1, lane_word(w3, 2 * J + 1),
                                                               site_pair(tab, kCtl, CQ), lane, v.fired, v.pol);
                        });
                        call += 2 * N;
                        frame_regs<N>(pr, pi, x, z, lane);
                        if (__any(nrm2 < 0x1p-200)) {
#pragma unroll
                            for (int i = 0; i < R; ++i) { pr[i] *= 0x1p100; pi[i] *= 0x1p100; }
                            nrm2 *= 0x1p200;
                            v.fired |= 1u << 31;
                        }
                        v.x = x; v.z = z;
                        store_words(words, seg, lane, v);
                    }
                }
            }
            // ---- read-out: the forward kernel's value; lambda = h' psi~ / N2
            basis_change<N, false>(pr, pi, a.pauli, lane);
            double tot = 0.0, val = 0.0;
#pragma unroll
            for (int i = 0; i < R; ++i) tot += pr[i] * pr[i] + pi[i] * pi[i];
            tot = group_sum<6>(tot);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const double hk = g.hd[lane | (i << 6)];
                val += (pr[i] * pr[i] + pi[i] * pi[i]) * hk;
                lr[i] = hk * pr[i] / tot; li[i] = hk * pi[i] / tot;
            }
            val = group_sum<6>(val) / tot + off_term;
            sum += val; sq += val * val;
            if (a.pauli) {
                basis_change<N, true>(pr, pi, a.pauli, lane);
                basis_change<N, true>(lr, li, a.pauli, lane);
            }
            // ---- reverse: blocks backwards; per block one loop over its segments (l = ld .. 1 sub-layers, 0 the encoding)
            for (int gi = 1; gi >= 0; --gi) {
                const int ldg = a.ld[gi];
                for (int b = a.nb[gi] - 1; b >= 0; --b) {
                    --blk; s -= ldg; col -= N; seg -= 1 + ldg;           // the block's first sub-layer, columns and segment
                    int l = ldg, cur = 0;
                    bool enter = true, have = false;
                    SegWords v{0u, 0u, 0, 0};
                    double acc[C::KW];
                    for (;;) {
                        if (enter) {
                            v = load_words(words, seg + l, lane);
                            if (v.fired >> 31) {
#pragma unroll
                                for (int i = 0; i < R; ++i) {
                                    pr[i] *= 0x1p-100; pi[i] *= 0x1p-100;
                                    lr[i] *= 0x1p100; li[i] *= 0x1p100;
                                }
                            }
                            frame_regs<N>(pr, pi, v.x, v.z, lane);
                            frame_regs<N>(lr, li, v.x, v.z, lane);
                            // frame_regs twice is (-1)^parity(x & z): the sign makes it the inverse.  psi and lambda share
                            // it, but a snapshot restores psi with its own sign, so it is not left to cancel
                            if (__popc((unsigned)(v.x & v.z)) & 1) {
#pragma unroll
                                for (int i = 0; i < R; ++i) { pr[i] = -pr[i]; pi[i] = -pi[i]; lr[i] = -lr[i]; li[i] = -li[i]; }
                            }
                            cur = l ? 3 * N : N;
                            have = false; enter = false;
#pragma unroll
                            for (int i = 0; i < C::KW; ++i) acc[i] = 0.0;
                        }
                        bool stopped = false;
                        if (l) {
                            const int sl = s + l - 1;
                            static_rfor<0, N>([&](auto jj) {
                                constexpr int J = decltype(jj)::value, CQ = (J + 1) % N, TQ = J;
                                relax_undo<N, CQ, N + 2 * J + 1, kCtl>(pr, pi, lr, li, tab, v.fired, v.pol, cur, have, stopped, lane,
                                                                       [] {});
                                relax_undo<N, TQ, N + 2 * J, kTgt>(pr, pi, lr, li, tab, v.fired, v.pol, cur, have, stopped, lane, [&] {
                                    apply_cnot<N, CQ, TQ>(pr, pi, lane);
                                    apply_cnot<N, CQ, TQ>(lr, li, lane);
                                });
                            });
                            static_rfor<0, N>([&](auto q) {
                                constexpr int Q = decltype(q)::value;
                                constexpr bool kSigned = Q < C::LB && !kSwapQubit<N, Q>;
                                relax_undo<N, Q, Q, kRot>(pr, pi, lr, li, tab, v.fired, v.pol, cur, have, stopped, lane, [&] {
                                    const double4 u = a.gates[2 * (sl * N + Q + N) + (kSigned ? (lane >> Q) & 1 : 0)];
                                    su2_inverse_with_inner<N, Q>(pr, pi, lr, li, u, lane, acc[3 * Q], acc[3 * Q + 1], acc[3 * Q + 2]);
                                });
                            });
                        } else {
                            static_rfor<0, N>([&](auto q) {
                                constexpr int Q = decltype(q)::value;
                                relax_undo<N, Q, Q, kEnc>(pr, pi, lr, li, tab, v.fired, v.pol, cur, have, stopped, lane, [&] {
                                    const double2 c = csr[col + Q];
                                    acc[Q] = pauli_x_inner<N, Q>(pr, pi, lr, li);
                                    apply_rx<N, Q>(pr, pi, c.x, -c.y);
                                    apply_rx<N, Q>(lr, li, c.x, -c.y);
                                });
                            });
                        }
                        if (cur == 0) {                                  // the segment is done: its sums into the item's record
                            if (l) {
                                const int vi = butterfly_sum<C::KW>(acc, lane);
                                if (butterfly_owner<C::KW>(lane) && vi < 3 * N) {
                                    double* p = rec_w + (long)(s + l - 1) * 3 * N + vi;
                                    *p = first ? acc[0] : *p + acc[0];
                                }
                                --l; enter = true;
                                continue;
                            }
                            double gx[C::KX];
#pragma unroll
                            for (int i = 0; i < C::KX; ++i) gx[i] = i < N ? acc[i] : 0.0;
                            lane_reduce<C::KX, C::LB>(gx, lane);         // lane j < KX holds value j
                            if (lane < N) {
                                double* p = rec + col + lane;
                                *p = first ? gx[0] : *p + gx[0];
                            }
                            break;
                        }
                        // a fired site: psi from before the jump -- the block's snapshot walked forward to site cur - 1
                        // (QHEA_DEVICE_GRAD_SKIP_REWALK: timing builds only, wrong results -- the share of the re-walks)
#ifndef QHEA_DEVICE_GRAD_SKIP_REWALK
#pragma unroll
                        for (int i = 0; i < R; ++i) {
                            pr[i] = snap[((long)blk * 2 * R + i) * 64];
                            pi[i] = snap[((long)blk * 2 * R + R + i) * 64];
                        }
                        replay_enc<N>(pr, pi, tab, csr + col, load_words(words, seg, lane), l ? kAllSites : cur - 1, lane);
                        for (int j = 1; j <= l; ++j)
                            replay_sub<N>(pr, pi, tab, a.gates, s + j - 1, load_words(words, seg + j, lane), j == l ? cur - 1 : kAllSites,
                                          lane);
#endif
                        have = true;
                    }
                }
            }
        }
        if (lane == 0) a.partial[item] = make_double2(sum, sq);
    }
}

__global__ __launch_bounds__(256) void device_grad_tables_kernel(DevGradTable t, DevGradTable* __restrict__ out,
                                                                 const double* __restrict__ diag, double co, int n,
                                                                 double* __restrict__ buf) {
    jump_tables_body(t, out, diag, co, n, buf);
}

int launch_device_grad(int n, const NoisyGradArgs& g, const DevGradArgs& d, hipStream_t st) {
    const dim3 grid((unsigned)(d.waves / kDevGradWaves + (d.waves % kDevGradWaves ? 1 : 0))), block(64 * kDevGradWaves);
    switch (n) {
        case 7: hipLaunchKernelGGL(device_grad_wave_kernel<7>, grid, block, 0, st, g, d); break;
        case 8: hipLaunchKernelGGL(device_grad_wave_kernel<8>, grid, block, 0, st, g, d); break;
        case 9: hipLaunchKernelGGL(device_grad_wave_kernel<9>, grid, block, 0, st, g, d); break;
        default: return QHEA_EUNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

// ---- the unit of hea_noise_jump_grad.hpp's host body ------------------------------------------------------------------------------------

struct JumpWaveUnit {
    using Table = DevGradTable;
    using Args = DevGradArgs;
    using Snap = double;
    static constexpr GradUnit unit{7, 9, kDevGradTile, nullptr};         // the layout's qubit range and tile
    static JumpTable<kJumpMaxWires>& jump(Table& t) { return t; }
    static const JumpTable<kJumpMaxWires>& jump(const Table& t) { return t; }
    static constexpr int cap(int) { return kDevGradMaxWaves; }
    static long words_stride(long segs) { return segs * 4 * 64; }
    static long snap_stride(long blocks, int n) { return blocks * (2L << n); }       // 2 R doubles on 64 lanes per block
    static void launch_tables(const Table& tb, Table* out, const double* diag, double co, int n, double* buf, hipStream_t st) {
        hipLaunchKernelGGL(device_grad_tables_kernel, dim3(1), dim3(256), 0, st, tb, out, diag, co, n, buf);
    }
    static int launch(int n, const NoisyGradArgs& g, Args d, int waves, hipStream_t st) {
        d.waves = waves;
        return launch_device_grad(n, g, d, st);
    }
};

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

int qhea_device_noise_singular_site(int n, const qhea_device_noise* dn, int* site, int* wire) {
    const int rc = device_noise_check(n, dn);
    if (rc != QHEA_OK) return rc;
    double flat[4 * QHEA_MAX_QUBITS * 2];
    jump_tables(n, dn, flat);
    for (int s = 0; s < 4; ++s)
        for (int q = 0; q < n; ++q)
            if (1.0 - flat[((size_t)s * n + q) * 2] == 0.0) {
                if (site) *site = s;
                if (wire) *wire = q;
                return 1;
            }
    return QHEA_OK;
}

size_t qhea_model_noisy_device_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling) {
    return jump_grad_workspace_bytes<JumpWaveUnit>(desc, batch, sampling);
}

int qhea_model_loss_grad_noisy_device(const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch,
                                      const double* trunk, const double* y, const double* params, const double* ham_diag,
                                      const qhea_device_noise* dn, const qhea_sampling* sampling, double inv_batch_total,
                                      double* grad, double* pred, void* workspace, size_t workspace_bytes, void* stream) {
    return jump_grad_loss_grad<JumpWaveUnit>(desc, row0, batch, branch, trunk, y, params, ham_diag, dn, sampling, inv_batch_total,
                                             grad, pred, workspace, workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_device(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                        const double* branch, const double* trunk, const double* y, double* params,
                                        const double* ham_diag, const qhea_device_noise* dn, const qhea_sampling* sampling,
                                        const double* inv_batch_total, double* grad, int64_t grad_stride, double* exp_avg,
                                        double* exp_avg_sq, int64_t first_step, double lr, double beta1, double beta2, double eps,
                                        double weight_decay, void* workspace, size_t workspace_bytes, void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return jump_grad_train_steps<JumpWaveUnit>(desc, call, ham_diag, dn, sampling, lr);
}

}  // extern "C"
