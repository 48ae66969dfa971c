// hea_noise_device.hip -- qhea_model_forward_noisy_device: the model forward under the calibrated device noise model
// (qhea_device_noise) estimated from quantum-jump (Monte-Carlo wave-function) trajectories, n = 2..9, expectation mode and shot
// mode.  The quantity, the unravelling, the random stream and the summation orders are the contract stated in
// include/quanonet_hea.h; tests/device_traj_reference.py replays them gate by gate.
//
// Two kernels, in the layouts of the uniform trajectory units:
//   n = 2..6   one amplitude per lane, 64 / 2^n trajectories of one row per wave (hea_noise.hip);
//   n = 7..9   one wave per trajectory in Cfg<N>'s register layout (hea_noise_wide.hip): wires 0..5 on lane bits, 6..8 in registers.
// A work item is a (row, tile of kTile trajectories) pair as there; noisy_finish_kernel adds a row's tiles.
//
// What relaxation changes against the Pauli kernels:
//   * The state is carried UNNORMALISED with its squared norm beside it (nrm2).  A damping site needs M, the masked sum of
//     |psi_k|^2 over the amplitudes whose wire is |1>: the jump fires iff u nrm2 < gamma M (u < gamma P1 with P1 = M / nrm2), a
//     jump leaves nrm2 = M, no jump scales the |1> half by sqrt(1 - gamma) and leaves nrm2 - gamma M.  So a site costs no
//     division and no square root; the read-out divides by the state's own sum of squares once per trajectory.  A power-of-two
//     rescale behind a segment keeps the numbers in range (exact, so invisible in the result).
//   * The Pauli frame (X mask, Z mask) stays unapplied across the sites of a segment: Z bits change no population, an X bit on
//     the wire swaps which stored bit value is |1> (the polarity of the mask above), the lowering operator acts on the stored
//     state with that polarity up to a global sign, and dephasing toggles a Z bit.
//   * A jump sits behind every CNOT slot, so the ring is applied CNOT by CNOT (a one-bit exchange and a select each) and not as
//     one gather; the frame is conjugated through each as before.
//   * A fired jump is rare: its exchange is guarded by __any.
// Philox calls are shared as in segment_codes: lane c of a slot (or of the wave) computes call c of the segment -- the encoding
// sites of a block, the rotation sites of a sub-layer, or the 2 n calls of its ring -- and reduces it to a code (Pauli in bits
// 0..3, dephasing in bit 4) and the jump's word; every site reads the two from that lane.  The per-call thresholds and the
// per-site (gamma, sqrt(1 - gamma)) come from a small table in the workspace that one prep launch fills from its arguments: the
// trajectory kernels read it by wave-uniform addresses, so the constants live in scalar registers only while a site uses them.
//
// The work item, apply_frame, frame_regs, wave_scan, uniform, u of the cdf search and shot_value are hea_noise_traj.hpp's, shared
// with the uniform units.  The table (DevTable), the body of the prep kernel that writes it, site_pair, group_sum, jump_u,
// draw_code and the body of the entry point (jump_forward, around traj_open and traj_finish) are hea_noise_jump.hpp's, shared
// with hea_noise_device_wide.hip.  Where a kernel below still spells out what hea_noise.hip or hea_noise_wide.hip also hold (the
// lane butterflies, the basis change, the cdf searches, the slot fold, the wave kernel's work item and shot words), the shared
// form changed its device code (profiles/r25_device_code_identity.txt).
#include <climits>
#include <cmath>
#include <cstdint>

#include "hea_noise_jump.hpp"

namespace qhea {
namespace {

constexpr int kJumpWaves = 4;               // waves per workgroup (independent; no LDS, no barrier)

// ---- device helpers of this unit ----------------------------------------------------------------------------------------------------

// This lane's call of a segment: call0 + c for c < cnt, template entry tbase + c of the table.  code = the sampled Pauli
// (0 none; one qubit 1..3; RING, even calls: the pair 1..15) | dephasing << 4; w3 = the jump's word.  a.thr1 == 0: an ideal
// setting, nothing is drawn.
template <bool RING>
__device__ __forceinline__ void site_draws(const NoiseArgs& a, const DevTable* __restrict__ tab, unsigned call0, int tbase, int cnt,
                                           int c, unsigned traj, unsigned long long row, unsigned& code, unsigned& w3) {
    code = 0; w3 = 0;
    if (a.thr1 == 0 || c >= cnt) return;
    const uint4 w = philox(make_uint4(call0 + (unsigned)c, traj, (unsigned)row, (unsigned)(row >> 32)), a.key0, a.key1);
    draw_code(tab, tbase + c, w, (RING && !(c & 1)) ? 15u : 3u, code, w3);
}

// The read-out's arguments from the table, behind the fence of site_pair: with one wave per trajectory the circuit loop leaves no
// scalar registers for values that are only used behind it, and kernel arguments would be parked in vector lanes meanwhile.
struct ReadoutArgs { double off, co; const double* diag; unsigned L, pauli; };
__device__ __forceinline__ ReadoutArgs readout_args(const DevTable* __restrict__ tab) {
    int fence = 0;
    asm volatile("" : "+s"(fence));
    const DevTable* t = reinterpret_cast<const DevTable*>(reinterpret_cast<const char*>(tab) + fence);
    return {t->off, t->co, t->diag, t->L, t->pauli};
}

// ---- n = 2..6: one amplitude per lane ----------------------------------------------------------------------------------------------

// dephasing and damping of one site on wire q; c, w3: the site's code and jump word, (g, s) = (gamma, sqrt(1 - gamma))
template <int N>
__device__ __forceinline__ void relax_lane(double& re, double& im, double& nrm2, int x, int& z, int q, unsigned c, unsigned w3,
                                           double2 gs, int k, int lane) {
    const double g = gs.x, s = gs.y;
    z ^= (int)((c >> 4) & 1u) << q;
    if (g > 0.0) {                                                       // wave-uniform: a table entry
        const bool one = ((k ^ x) >> q) & 1;                             // this amplitude has the wire in |1>
        const double M = group_sum<N>(one ? re * re + im * im : 0.0);
        const bool fire = jump_u(w3) * nrm2 < g * M;
        if (__any(fire)) {
            const double pr = __shfl(re, lane ^ (1 << q)), pi = __shfl(im, lane ^ (1 << q));
            if (fire) { re = one ? 0.0 : pr; im = one ? 0.0 : pi; nrm2 = M; }
        }
        if (!fire) {
            const double f = one ? s : 1.0;
            re *= f; im *= f;
            nrm2 -= g * M;
        }
    }
}

__device__ __forceinline__ void rescale_lane(double& re, double& im, double& nrm2) {
    if (__any(nrm2 < 0x1p-200)) {
        const double f = nrm2 < 0x1p-200 ? 0x1p100 : 1.0;
        re *= f; im *= f; nrm2 *= f * f;
    }
}

template <int N>
__global__ __launch_bounds__(64 * kJumpWaves) void device_traj_lane_kernel(NoiseArgs a, const DevTable* __restrict__ tab,
                                                                           const double* __restrict__ hd) {
    constexpr int D = 1 << N, SL = 64 / D;
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * kJumpWaves + (threadIdx.x >> 6);
    if (item >= a.B * a.tiles) return;                                   // whole waves
    const WorkItem wi = work_item(a, item);
    const int k = lane & (D - 1), base = lane - k, slot = lane / D;
    const double hk = a.shots ? 0.0 : hd[k];
    const double off_term = (a.shots || a.diag) ? 0.0 : a.off;

    double sum = 0.0, sq = 0.0;
    for (int it = 0; it < wi.tcount; it += SL) {
        const int tj = it + slot;
        const unsigned traj = (unsigned)(wi.t0 + tj);
        double re = k == 0 ? 1.0 : 0.0, im = 0.0, nrm2 = 1.0;
        unsigned call = 0, code, w3;
        int s = 0, col = 0;
        for (int g = 0; g < 2; ++g) {
            for (int b = 0; b < a.nb[g]; ++b) {
                // per wire: encoding RX, then site ENC (Pauli, dephasing, jump)
                site_draws<false>(a, tab, call, 0, N, k, traj, wi.row, code, w3);
                int x = 0, z = 0;
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    const double2 c = wi.csr[col + q];
                    const double pr = __shfl(re, lane ^ (1 << q)), pi = __shfl(im, lane ^ (1 << q));
                    const double nr = c.x * re + c.y * pi, ni = c.x * im - c.y * pr;
                    re = nr; im = ni;
                    const unsigned cq = __shfl(code, base + q);
                    x ^= pauli_x(cq & 3u, q); z ^= pauli_z(cq & 3u, q);
                    relax_lane<N>(re, im, nrm2, x, z, q, cq, __shfl(w3, base + q), site_pair(tab, kEnc, q), k, lane);
                }
                apply_frame(re, im, x, z, k, base);
                rescale_lane(re, im, nrm2);
                col += N; call += N;
                for (int l = 0; l < a.ld[g]; ++l, ++s) {
                    site_draws<false>(a, tab, call, N, N, k, traj, wi.row, code, w3);
                    x = 0; z = 0;
#pragma unroll
                    for (int q = 0; q < N; ++q) {                        // fused RY RZ RY per wire, then site ROT
                        const double4 v = a.gates[2 * (s * N + q + N) + ((k >> q) & 1)];
                        const double pr = __shfl(re, lane ^ (1 << q)), pi = __shfl(im, lane ^ (1 << q));
                        const double nr = v.x * re - v.y * im + v.z * pr - v.w * pi;
                        const double ni = v.x * im + v.y * re + v.z * pi + v.w * pr;
                        re = nr; im = ni;
                        const unsigned cq = __shfl(code, base + q);
                        x ^= pauli_x(cq & 3u, q); z ^= pauli_z(cq & 3u, q);
                        relax_lane<N>(re, im, nrm2, x, z, q, cq, __shfl(w3, base + q), site_pair(tab, kRot, q), k,
                                      lane);
                    }
                    call += N;
                    site_draws<true>(a, tab, call, 2 * N, 2 * N, k, traj, wi.row, code, w3);
#pragma unroll
                    for (int j = 0; j < N; ++j) {                        // slot j: CNOT(c -> t), pair Pauli, TGT of t, CTL of c
                        const int c = (j + 1) % N, t = j;
                        const double pr = __shfl(re, lane ^ (1 << t)), pi = __shfl(im, lane ^ (1 << t));
                        const bool on = (k >> c) & 1;
                        re = on ? pr : re; im = on ? pi : im;
                        x ^= ((x >> c) & 1) << t;
                        z ^= ((z >> t) & 1) << c;
                        const unsigned c0 = __shfl(code, base + 2 * j), c1 = __shfl(code, base + 2 * j + 1);
                        const unsigned p = c0 & 15u;
                        x ^= pauli_x(p >> 2, c) | pauli_x(p & 3u, t);
                        z ^= pauli_z(p >> 2, c) | pauli_z(p & 3u, t);
                        relax_lane<N>(re, im, nrm2, x, z, t, c0, __shfl(w3, base + 2 * j), site_pair(tab, kTgt, t), k,
                                      lane);
                        relax_lane<N>(re, im, nrm2, x, z, c, c1, __shfl(w3, base + 2 * j + 1), site_pair(tab, kCtl, c), k, lane);
                    }
                    call += 2 * N;
                    apply_frame(re, im, x, z, k, base);
                    rescale_lane(re, im, nrm2);
                }
            }
        }
        // the lane index behind a fence: what the read-out derives from it (bit masks, shot-mode selects) is computed here, per
        // trajectory, and not kept in scalar registers across the circuit loop
        int rl = lane;
        asm volatile("" : "+v"(rl));
        const int rk = rl & (D - 1), rbase = rl - rk;
        // noiseless basis change of the X / Y read-outs: H, or H S^dagger, on every wire
        if (a.pauli != QHEA_PAULI_Z) {
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const int bit = (rk >> q) & 1;
                if (a.pauli == QHEA_PAULI_Y && bit) { const double t = re; re = im; im = -t; }
                const double pr = __shfl(re, rl ^ (1 << q)), pi = __shfl(im, rl ^ (1 << q));
                re = M_SQRT1_2 * (bit ? pr - re : re + pr);
                im = M_SQRT1_2 * (bit ? pi - im : im + pi);
            }
        }
        const double pk = re * re + im * im;
        const double tot = group_sum<N>(pk);
        double v;
        if (!a.shots) {
            v = group_sum<N>(pk * hk) / tot + off_term;
        } else {
            // one measured bitstring: u against the cdf in index order, then the n readout flips of its own bits
            const uint4 w0 = philox(make_uint4(a.L, traj, (unsigned)wi.row, (unsigned)(wi.row >> 32)), a.key0, a.key1);
            const uint4 w1 = philox(make_uint4(a.L + 1, traj, (unsigned)wi.row, (unsigned)(wi.row >> 32)), a.key0, a.key1);
            const double u = unit_double(w0.x, w0.y);
            const double ut = u * tot;
            double acc = 0.0;
            int out = -1, last = 0;
            for (int j = 0; j < D; ++j) {
                const double pj = __shfl(pk, rbase + j);
                acc += pj;
                if (out < 0 && ut < acc) out = j;
                if (pj > 0.0) last = j;
            }
            if (out < 0) out = last;
            const unsigned rw[6] = {w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
            int flips = 0;
#pragma unroll
            for (int i = 0; i < N; ++i)
                flips |= (unsigned long long)rw[i] < tab->rthr[i][(out >> i) & 1] ? 1 << i : 0;
            v = shot_value<N>(a.diag, a.off, a.co, out ^ flips);
        }
        if (tj < wi.tcount) { sum += v; sq += v * v; }
    }
    double S = 0.0, Q = 0.0;
#pragma unroll
    for (int j = 0; j < SL; ++j) { S += __shfl(sum, j * D); Q += __shfl(sq, j * D); }
    if (lane == 0) a.partial[item] = make_double2(S, Q);
}

// ---- n = 7..9: one wave, 2^(n-6) amplitudes per lane ---------------------------------------------------------------------------------

// dephasing and damping of one site on wire Q; x, z, c, w3 wave-uniform
template <int N, int Q>
__device__ __forceinline__ void relax_regs(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], double& nrm2, int x, int& z, unsigned c,
                                           unsigned w3, double2 gs, int lane) {
    using C = Cfg<N>;
    const double g = gs.x, s = gs.y;
    constexpr int R = C::R;
    z ^= (int)((c >> 4) & 1u) << Q;
    if (g > 0.0) {
        const int xq = (x >> Q) & 1;
        bool one[R];
        double M = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            one[r] = ((Q < C::LB ? (lane >> Q) : (r >> (Q >= C::LB ? Q - C::LB : 0))) & 1) != xq;
            M += one[r] ? re[r] * re[r] + im[r] * im[r] : 0.0;
        }
        M = group_sum<6>(M);
        const bool fire = jump_u(w3) * nrm2 < g * M;                     // the same in every lane
        if (__any(fire)) {
            if constexpr (Q < C::LB) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double pr = xchg<(1 << Q)>(re[r]), pi = xchg<(1 << Q)>(im[r]);
                    re[r] = one[r] ? 0.0 : pr; im[r] = one[r] ? 0.0 : pi;
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
            nrm2 = M;
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double f = one[r] ? s : 1.0;
                re[r] *= f; im[r] *= f;
            }
            nrm2 -= g * M;
        }
    }
}

template <int N>
__device__ __forceinline__ void rescale_regs(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], double& nrm2) {
    if (__any(nrm2 < 0x1p-200)) {
#pragma unroll
        for (int r = 0; r < Cfg<N>::R; ++r) { re[r] *= 0x1p100; im[r] *= 0x1p100; }
        nrm2 *= 0x1p200;
    }
}

__device__ __forceinline__ unsigned lane_word(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane((int)v, l); }

template <int N>
__global__ __launch_bounds__(64 * kJumpWaves) void device_traj_wave_kernel(NoiseArgs a, const DevTable* __restrict__ tab,
                                                                           const double* __restrict__ hd) {
    using C = Cfg<N>;
    constexpr int R = C::R;
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * kJumpWaves + (threadIdx.x >> 6);
    if (item >= a.B * a.tiles) return;                                   // whole waves
    // (written out, not work_item(): with it this kernel's device code changes; the same holds for u of the cdf search below)
    const long r = item / a.tiles;
    const long t0 = (item - r * a.tiles) * (long)kTile;
    const int tcount = (int)(a.T - t0 < kTile ? a.T - t0 : kTile);
    const unsigned long long row = (unsigned long long)(a.row0 + r);
    const double2* csr = a.cs + r * a.E;

    double hk[R];
#pragma unroll
    for (int i = 0; i < R; ++i) hk[i] = a.shots ? 0.0 : hd[lane | (i << 6)];
    const double off_term = (a.shots || a.diag) ? 0.0 : a.off;

    double sum = 0.0, sq = 0.0;
    for (int tj = 0; tj < tcount; ++tj) {
        const unsigned traj = (unsigned)(t0 + tj);
        double re[R], im[R], nrm2 = 1.0;
#pragma unroll
        for (int i = 0; i < R; ++i) { re[i] = 0.0; im[i] = 0.0; }
        re[0] = lane == 0 ? 1.0 : 0.0;
        unsigned call = 0, code, w3;
        int s = 0, col = 0;
        for (int g = 0; g < 2; ++g) {
            for (int b = 0; b < a.nb[g]; ++b) {
                site_draws<false>(a, tab, call, 0, N, lane, traj, row, code, w3);
                int x = 0, z = 0;
                static_for<0, N>([&](auto q) {                           // encoding RX, then site ENC
                    constexpr int Q = decltype(q)::value;
                    const double2 c = csr[col + Q];
                    apply_rx<N, Q>(re, im, c.x, c.y);
                    const unsigned cq = lane_word(code, Q);
                    x ^= pauli_x(cq & 3u, Q); z ^= pauli_z(cq & 3u, Q);
                    relax_regs<N, Q>(re, im, nrm2, x, z, cq, lane_word(w3, Q), site_pair(tab, kEnc, Q), lane);
                });
                frame_regs<N>(re, im, x, z, lane);
                rescale_regs<N>(re, im, nrm2);
                col += N; call += N;
                for (int l = 0; l < a.ld[g]; ++l, ++s) {
                    site_draws<false>(a, tab, call, N, N, lane, traj, row, code, w3);
                    x = 0; z = 0;
                    static_for<0, N>([&](auto q) {                       // fused RY RZ RY, then site ROT
                        constexpr int Q = decltype(q)::value;
                        constexpr bool kSigned = Q < C::LB && !kSwapQubit<N, Q>;   // the lane's variant of the gate table
                        const double4 v = a.gates[2 * (s * N + Q + N) + (kSigned ? (lane >> Q) & 1 : 0)];
                        apply_su2<N, Q>(re, im, v.x, v.y, v.z, v.w);
                        const unsigned cq = lane_word(code, Q);
                        x ^= pauli_x(cq & 3u, Q); z ^= pauli_z(cq & 3u, Q);
                        relax_regs<N, Q>(re, im, nrm2, x, z, cq, lane_word(w3, Q), site_pair(tab, kRot, Q), lane);
                    });
                    call += N;
                    site_draws<true>(a, tab, call, 2 * N, 2 * N, lane, traj, row, code, w3);
                    static_for<0, N>([&](auto jj) {                      // slot j: CNOT(c -> t), pair Pauli, TGT of t, CTL of c
                        constexpr int J = decltype(jj)::value, CQ = (J + 1) % N, TQ = J;
                        apply_cnot<N, CQ, TQ>(re, im, lane);
                        x ^= ((x >> CQ) & 1) << TQ;
                        z ^= ((z >> TQ) & 1) << CQ;
                        const unsigned c0 = lane_word(code, 2 * J), c1 = lane_word(code, 2 * J + 1);
                        const unsigned p = c0 & 15u;
                        x ^= pauli_x(p >> 2, CQ) | pauli_x(p & 3u, TQ);
                        z ^= pauli_z(p >> 2, CQ) | pauli_z(p & 3u, TQ);
                        relax_regs<N, TQ>(re, im, nrm2, x, z, c0, lane_word(w3, 2 * J), site_pair(tab, kTgt, TQ),
                                          lane);
                        relax_regs<N, CQ>(re, im, nrm2, x, z, c1, lane_word(w3, 2 * J + 1), site_pair(tab, kCtl, CQ), lane);
                    });
                    call += 2 * N;
                    frame_regs<N>(re, im, x, z, lane);
                    rescale_regs<N>(re, im, nrm2);
                }
            }
        }
        int rl = lane;                                                   // behind a fence, as in the lane kernel's read-out
        asm volatile("" : "+v"(rl));
        const ReadoutArgs ro = readout_args(tab);
        basis_change<N, false>(re, im, (int)ro.pauli, rl);               // same probabilities as H / H S^dagger
        double pk[R], tot = 0.0;
#pragma unroll
        for (int i = 0; i < R; ++i) { pk[i] = re[i] * re[i] + im[i] * im[i]; tot += pk[i]; }
        tot = group_sum<6>(tot);
        double v;
        if (!a.shots) {
            v = 0.0;
#pragma unroll
            for (int i = 0; i < R; ++i) v += pk[i] * hk[i];
            v = group_sum<6>(v) / tot + off_term;
        } else {
            // calls L .. L + 2: u, then per bit the flip words against both thresholds (the outcome picks the direction)
            const int j = rl & 3;
            const uint4 w = philox(make_uint4(ro.L + (unsigned)j, traj, (unsigned)row, (unsigned)(row >> 32)), a.key0, a.key1);
            const unsigned wd[4] = {w.x, w.y, w.z, w.w};
            int m01 = 0, m10 = 0;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int i = 4 * j + h - 2;
                if (i >= 0 && i < N) {
                    if ((unsigned long long)wd[h] < tab->rthr[i][0]) m01 |= 1 << i;
                    if ((unsigned long long)wd[h] < tab->rthr[i][1]) m10 |= 1 << i;
                }
            }
            m01 = uniform(__shfl(m01, 0) | __shfl(m01, 1) | __shfl(m01, 2) | __shfl(m01, 3));
            m10 = uniform(__shfl(m10, 0) | __shfl(m10, 1) | __shfl(m10, 2) | __shfl(m10, 3));
            const double ut = __shfl(((double)(w.x >> 5) * 67108864.0 + (double)(w.y >> 6)) * 0x1p-53, 0) * tot;
            int out = -1, last = 0;
            double below = 0.0;                                          // cdf of the blocks of 64 before this one
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const double c = wave_scan(pk[i], rl);
                const unsigned long long hit = __ballot(ut < below + c), pos = __ballot(pk[i] > 0.0);
                if (out < 0 && hit) out = (i << 6) | (__ffsll(hit) - 1);
                if (pos) last = (i << 6) | (63 - __clzll(pos));
                below += __shfl(c, 63);
            }
            if (out < 0) out = last;
            v = shot_value<N>(ro.diag, ro.off, ro.co, out ^ ((out & m10) | (~out & m01)));
        }
        sum += v; sq += v * v;
    }
    if (lane == 0) a.partial[item] = make_double2(sum, sq);
}

// ---- prep: the table, and expectation mode's read-out weights -------------------------------------------------------------------------

__global__ __launch_bounds__(256) void device_tables_kernel(DevTable t, DevTable* __restrict__ out, const double* __restrict__ diag,
                                                            double co, int n, double* __restrict__ buf) {
    jump_tables_body(t, out, diag, co, n, buf);
}

int launch_device_traj(const NoiseArgs& a, int n, const DevTable* tab, const double* hd, hipStream_t st) {
    const long items = a.B * a.tiles;
    const dim3 grid((unsigned)((items + kJumpWaves - 1) / kJumpWaves)), block(64 * kJumpWaves);
    switch (n) {
        case 2: hipLaunchKernelGGL(device_traj_lane_kernel<2>, grid, block, 0, st, a, tab, hd); break;
        case 3: hipLaunchKernelGGL(device_traj_lane_kernel<3>, grid, block, 0, st, a, tab, hd); break;
        case 4: hipLaunchKernelGGL(device_traj_lane_kernel<4>, grid, block, 0, st, a, tab, hd); break;
        case 5: hipLaunchKernelGGL(device_traj_lane_kernel<5>, grid, block, 0, st, a, tab, hd); break;
        case 6: hipLaunchKernelGGL(device_traj_lane_kernel<6>, grid, block, 0, st, a, tab, hd); break;
        case 7: hipLaunchKernelGGL(device_traj_wave_kernel<7>, grid, block, 0, st, a, tab, hd); break;
        case 8: hipLaunchKernelGGL(device_traj_wave_kernel<8>, grid, block, 0, st, a, tab, hd); break;
        case 9: hipLaunchKernelGGL(device_traj_wave_kernel<9>, grid, block, 0, st, a, tab, hd); break;
        default: return QHEA_EUNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

// the uniform units' layout with the read-out region of the wide ones, then the table
constexpr TrajUnit kJumpUnit{QHEA_MIN_QUBITS, kJumpMaxWires, true, sizeof(DevTable)};

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

int qhea_device_noise_jump_tables(int n, const qhea_device_noise* dn, double* jump) {
    const int rc = device_noise_check(n, dn);
    if (rc != QHEA_OK) return rc;
    if (!jump) return QHEA_EINVAL;
    jump_tables(n, dn, jump);
    return QHEA_OK;
}

size_t qhea_model_noisy_device_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling) {
    return jump_workspace_bytes(kJumpUnit, desc, batch, sampling);
}

int qhea_model_forward_noisy_device(const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch,
                                    const double* trunk, const double* params, const double* ham_diag,
                                    const qhea_device_noise* dn, const qhea_sampling* sampling, double* pred, double* stderr_out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    return jump_forward(kJumpUnit, device_tables_kernel, launch_device_traj, desc, row0, batch, branch, trunk, params, ham_diag, dn,
                        sampling, pred, stderr_out, workspace, workspace_bytes, stream);
}

}  // extern "C"
