// hea_noise_wide.hip -- qhea_model_forward_noisy_wide: the noisy forward of hea_noise.hip for n = 7..12, where a state no longer
// sits one amplitude per lane.  Same quantity, same noise model, same random stream (include/quanonet_hea.h); what differs is
// where the state lives and, with it, the order of the floating-point sums, which the header states.
//
// A work item is one (row, tile) pair: the up-to-kTile trajectories of a tile run one after another, their values are added in
// trajectory order, and noisy_finish_kernel (hea_noise.hip) adds a row's tiles in tile order.
//
//   n = 7..9    one wave per item, the state in Cfg<N>'s layout (hea_device.hpp): index bits 0..5 on the lane, the rest in
//               2^(n-6) registers.  Gates are the wave-resident helpers (apply_rx, apply_su2, apply_ring, basis_change).
//   n = 10..12  one workgroup of 2^(n-4) threads per item, the state in LDS, a gate layer in the three passes of hea_lds.hpp
//               with the ring folded into the last pass's scatter.
//
// Noise.  RX is applied on its own (noise sits between it and the rotation, so there is no merge_rx fold).  One item runs one
// trajectory at a time, so a segment's sampled Paulis (the encoding of a block, or one sub-layer) are ONE X mask and ONE Z mask
// for the whole wave or workgroup, pushed through the ring by x_t ^= x_c, z_c ^= z_t as in hea_noise.hip and applied once behind
// the segment: psi'[k] = (-1)^parity(k & z) psi[k ^ x] (a Pauli string up to a global phase).  In registers the lane part of x
// is one gather per register, the register part a renaming and z a sign.  In LDS the frame costs no pass: k -> k ^ x is linear
// like the ring and the swizzle, so x is one more xor on the last pass's store base and z a sign on the values stored.  Lane k
// of the first wave computes the segment's Philox call k (at most n + 1 = 13 calls); the frame is built from those by shuffles
// and, in the LDS kernels, handed to the other waves through two words of LDS.
//
// Read-out.  Expectation mode adds p_k h(k) per lane or thread in register order, then over the wave by the xor butterfly
// (offsets 32 .. 1) and over a workgroup's waves in wave order; with ham_diag, h is the readout-confused table, which
// readout_mix_kernel builds by n two-point mixes (the O(4^n) loop of hea_noise.hip is out of reach here).  Shot mode scans
// |psi_k|^2 into a cdf (block offsets in order, a Hillis-Steele scan over lanes inside a block) and locates the first k with
// u < cdf[k] by ballots or a workgroup minimum.  Nothing depends on the batch, the grid or the chunking; no atomics.
//
// The work item, frame_regs, wave_scan, uniform, u of the cdf search and shot_value are hea_noise_traj.hpp's, shared with
// hea_noise_device.hip; ring_pull and the last pass's store behind the frame (store_framed) are hea_lds.hpp's, shared with
// hea_noise_device_wide.hip; the frames of a segment (enc_frame, sub_frame), readout_weight and the readout mix's launcher are
// hea_noise_traj.hpp's too, shared with hea_noise_grad.hip; the shot words, the LDS kernel and the mix kernel are this unit's.
#include <climits>
#include <cmath>
#include <cstdint>

#include "hea_lds.hpp"
#include "hea_noise_traj.hpp"

namespace qhea {
namespace {

constexpr int kWideWaves = 4;               // n = 7..9: waves per workgroup (independent; no LDS, no barrier)
constexpr int kWideLG = 4;                  // n = 10..12: gate qubits per pass, as the ideal forward (hea_lds.hip)

// shot mode's words (header: calls m .. m + 3): u of the cdf search and the n readout flips as a bit mask; whole wave
template <int N>
__device__ __forceinline__ void shot_words(const NoiseArgs& a, unsigned traj, unsigned long long row, int lane, double& u,
                                           int& flips) {
    const int j = lane & 3;
    const uint4 w = philox(make_uint4(((a.L + 1) >> 1) + (unsigned)j, traj, (unsigned)row, (unsigned)(row >> 32)), a.key0, a.key1);
    const unsigned wd[4] = {w.x, w.y, w.z, w.w};
    int mask = 0;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int i = 4 * j + h - 2;
        if (i >= 0 && i < N && (unsigned long long)wd[h] < a.thrq) mask |= 1 << i;
    }
    flips = uniform(__shfl(mask, 0) | __shfl(mask, 1) | __shfl(mask, 2) | __shfl(mask, 3));
    u = __shfl(unit_double(w.x, w.y), 0);
}

// ---- n = 7..9: one wave, 2^(n-6) amplitudes per lane -------------------------------------------------------------------------

template <int N>
__global__ __launch_bounds__(64 * kWideWaves) void noisy_wide_wave_kernel(NoiseArgs a, const double* __restrict__ hd) {
    using C = Cfg<N>;
    constexpr int R = C::R;
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * kWideWaves + (threadIdx.x >> 6);
    if (item >= a.B * a.tiles) return;                                   // whole waves
    const WorkItem wi = work_item(a, item);
    const int ring_src = ring_source<N>(lane, false);

    double hk[R];
#pragma unroll
    for (int i = 0; i < R; ++i) hk[i] = a.shots ? 0.0 : readout_weight<N>(a, hd, lane | (i << 6));
    const double off_term = (a.shots || hd) ? 0.0 : a.off;

    double sum = 0.0, sq = 0.0;
    for (int tj = 0; tj < wi.tcount; ++tj) {
        const unsigned traj = (unsigned)(wi.t0 + tj);
        double re[R], im[R];
#pragma unroll
        for (int i = 0; i < R; ++i) { re[i] = 0.0; im[i] = 0.0; }
        re[0] = lane == 0 ? 1.0 : 0.0;
        unsigned loc = 0;
        int s = 0, col = 0, x, z;
        for (int g = 0; g < 2; ++g) {
            for (int b = 0; b < a.nb[g]; ++b) {
                // encoding RX on every wire, then one-qubit depolarizing noise on every wire
                unsigned codes = segment_codes(a, loc, N, N, traj, wi.row, lane);
                static_for<0, N>([&](auto q) {
                    constexpr int Q = decltype(q)::value;
                    const double2 c = wi.csr[col + Q];
                    apply_rx<N, Q>(re, im, c.x, c.y);
                });
                enc_frame<N>(codes, loc, x, z);
                frame_regs<N>(re, im, x, z, lane);
                col += N; loc += N;
                for (int l = 0; l < a.ld[g]; ++l, ++s, loc += 2 * N) {
                    codes = segment_codes(a, loc, 2 * N, N, traj, wi.row, lane);
                    static_for<0, N>([&](auto q) {                       // fused RY RZ RY per wire
                        constexpr int Q = decltype(q)::value;
                        constexpr bool kSigned = Q < C::LB && !kSwapQubit<N, Q>;   // the lane's variant of the gate table
                        const double4 v = a.gates[2 * (s * N + Q + N) + (kSigned ? (lane >> Q) & 1 : 0)];
                        apply_su2<N, Q>(re, im, v.x, v.y, v.z, v.w);
                    });
                    sub_frame<N>(codes, loc, x, z);
                    apply_ring<N, false>(re, im, lane, ring_src);
                    frame_regs<N>(re, im, x, z, lane);
                }
            }
        }
        basis_change<N, false>(re, im, a.pauli, lane);                   // same probabilities as H / H S^dagger
        double pk[R];
#pragma unroll
        for (int i = 0; i < R; ++i) pk[i] = re[i] * re[i] + im[i] * im[i];
        double v;
        if (!a.shots) {
            v = 0.0;
#pragma unroll
            for (int i = 0; i < R; ++i) v += pk[i] * hk[i];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
            v += off_term;
        } else {
            double u;
            int flips, out = -1, last = 0;
            shot_words<N>(a, traj, wi.row, lane, u, flips);
            double below = 0.0;                                          // cdf of the blocks of 64 before this one
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const double c = wave_scan(pk[i], lane);
                const unsigned long long hit = __ballot(u < below + c), pos = __ballot(pk[i] > 0.0);
                if (out < 0 && hit) out = (i << 6) | (__ffsll(hit) - 1);
                if (pos) last = (i << 6) | (63 - __clzll(pos));
                below += __shfl(c, 63);
            }
            if (out < 0) out = last;
            v = shot_value<N>(a.diag, a.off, a.co, out ^ flips);
        }
        sum += v; sq += v * v;
    }
    if (lane == 0) a.partial[item] = make_double2(sum, sq);
}

// ---- n = 10..12: one workgroup, the state in LDS --------------------------------------------------------------------------------

struct WideScratch {                        // behind the state
    double red[4];                          // per-wave sums (at most 4 waves)
    int lo[4], hi[4];                       // per-wave first hit / last positive index
    int frame[2];                           // the segment's frame: phys(x), and z pulled back through the ring where there is one
    int flips, pad;
    double u;
};

// the gate layer with a segment's frame behind it (noisy_layer) and the workgroup sum (wide_block_sum): hea_lds.hpp, shared
// with hea_noise_grad_lds.hip; the frame is sc->frame, written by thread 0 before the layer

template <int N>
__global__ __launch_bounds__((LCfg<N, kWideLG>::T)) void noisy_wide_lds_kernel(NoiseArgs a, const double* __restrict__ hd) {
    constexpr int LG = kWideLG, M = 1 << LG;
    using L = LCfg<N, LG>;
    extern __shared__ __attribute__((aligned(16))) char wide_lds[];
    double2* psi = reinterpret_cast<double2*>(wide_lds);
    WideScratch* sc = reinterpret_cast<WideScratch*>(wide_lds + L::STATE_BYTES);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long item = blockIdx.x;
    const WorkItem wi = work_item(a, item);
    Bases<N, LG> bs;
    bs.init(t);
    const int tpl = thread_part<Pass<N, L::NP - 1, LG>::A, LG>(t);
    const double off_term = (a.shots || hd) ? 0.0 : a.off;

    double sum = 0.0, sq = 0.0;
    for (int tj = 0; tj < wi.tcount; ++tj) {
        const unsigned traj = (unsigned)(wi.t0 + tj);
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int p = t + j * L::T;
            psi[p] = make_double2(p == 0 ? 1.0 : 0.0, 0.0);              // |0..0>: phys(0) = 0
        }
        __syncthreads();
        unsigned loc = 0;
        int s = 0, col = 0;
        for (int g = 0; g < 2; ++g) {
            for (int b = 0; b < a.nb[g]; ++b) {
                if (wave == 0) {
                    int x, z;
                    enc_frame<N>(segment_codes(a, loc, N, N, traj, wi.row, lane), loc, x, z);
                    if (t == 0) { sc->frame[0] = phys<LG>(x); sc->frame[1] = z; }
                }
                noisy_layer<N, false, LG>(psi, bs, tpl, sc->frame, [&](int q) { return rx_su2(wi.csr[col + q]); });
                col += N; loc += N;
                for (int l = 0; l < a.ld[g]; ++l, ++s, loc += 2 * N) {
                    if (wave == 0) {
                        int x, z;
                        sub_frame<N>(segment_codes(a, loc, 2 * N, N, traj, wi.row, lane), loc, x, z);
                        if (t == 0) { sc->frame[0] = phys<LG>(x); sc->frame[1] = ring_pull<N>(z); }
                    }
                    noisy_layer<N, true, LG>(psi, bs, tpl, sc->frame, [&](int q) { return a.gates[2 * ((s + 1) * N + q)]; });
                }
            }
        }
        if (a.pauli != QHEA_PAULI_Z) {                                   // same probabilities as H / H S^dagger
            constexpr double kR = 0.70710678118654752440;
            const double4 ub = a.pauli == QHEA_PAULI_X ? make_double4(kR, 0.0, kR, 0.0) : make_double4(kR, 0.0, 0.0, -kR);
            if (t == 0) { sc->frame[0] = 0; sc->frame[1] = 0; }
            noisy_layer<N, false, LG>(psi, bs, tpl, sc->frame, [&](int) { return ub; });
        }
        if (a.shots && wave == 0) {
            double u;
            int flips;
            shot_words<N>(a, traj, wi.row, lane, u, flips);
            if (t == 0) { sc->u = u; sc->flips = flips; }
        }
        // thread t reads the 16 consecutive basis states 16 t .. 16 t + 15
        c2 v[M];
        load_group<N, 0, false, LG>(psi, bs.plain[0], v);
        double pk[M];
#pragma unroll
        for (int j = 0; j < M; ++j) pk[j] = v[j].x * v[j].x + v[j].y * v[j].y;
        double val;
        if (!a.shots) {
            val = 0.0;
#pragma unroll
            for (int j = 0; j < M; ++j) val += pk[j] * readout_weight<N>(a, hd, (t << LG) | j);
            val = wide_block_sum<L::NW>(val, sc->red) + off_term;
        } else {
            double c[M];
            c[0] = pk[0];
#pragma unroll
            for (int j = 1; j < M; ++j) c[j] = c[j - 1] + pk[j];
            const double inc = wave_scan(c[M - 1], lane);
            double before = __shfl_up(inc, 1);
            if (lane == 0) before = 0.0;
            if (lane == 63) sc->red[wave] = inc;
            __syncthreads();                                             // red, u, flips
            double below = 0.0;
            for (int w = 0; w < wave; ++w) below += sc->red[w];
            below += before;
            const double u = sc->u;
            int lo = INT_MAX, hi = -1;
#pragma unroll
            for (int j = M - 1; j >= 0; --j) {
                if (u < below + c[j]) lo = (t << LG) | j;
                if (pk[j] > 0.0 && hi < 0) hi = (t << LG) | j;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const int l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
                lo = l2 < lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
            }
            if (lane == 0) { sc->lo[wave] = lo; sc->hi[wave] = hi; }
            __syncthreads();
            for (int w = 0; w < L::NW; ++w) {
                lo = sc->lo[w] < lo ? sc->lo[w] : lo;
                hi = sc->hi[w] > hi ? sc->hi[w] : hi;
            }
            const int out = lo != INT_MAX ? lo : (hi < 0 ? 0 : hi);
            val = shot_value<N>(a.diag, a.off, a.co, out ^ sc->flips);
        }
        sum += val; sq += val * val;
        __syncthreads();                                                 // psi and the scratch are rewritten
    }
    if (t == 0) a.partial[item] = make_double2(sum, sq);
}

// ham_diag under the readout confusion: bit by bit, h <- (1 - q) h + q h[k ^ bit]; stage i writes half i & 1 of buf[2 * 2^n],
// the table ends in half (n - 1) & 1.  One workgroup.
__global__ __launch_bounds__(256) void readout_mix_kernel(const double* __restrict__ diag, double q, int n, double* buf) {
    const int D = 1 << n;
    const double* src = diag;
    for (int i = 0; i < n; ++i) {
        double* dst = buf + (i & 1) * D;
        for (int k = threadIdx.x; k < D; k += 256) dst[k] = (1.0 - q) * src[k] + q * src[k ^ (1 << i)];
        __syncthreads();
        src = dst;
    }
}

template <int N>
int launch_wide(const NoiseArgs& a, const double* hd, hipStream_t st) {
    const long items = a.B * a.tiles;
    if constexpr (N <= 9) {
        hipLaunchKernelGGL(noisy_wide_wave_kernel<N>, dim3((unsigned)((items + kWideWaves - 1) / kWideWaves)), dim3(64 * kWideWaves),
                           0, st, a, hd);
        return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
    } else {
        using L = LCfg<N, kWideLG>;
        constexpr size_t smem = L::STATE_BYTES + sizeof(WideScratch);
        return launch_dynamic_lds(noisy_wide_lds_kernel<N>, dim3((unsigned)items), dim3(L::T), smem, st, a, hd);
    }
}

// ham_diag goes through readout_mix_kernel first where the kernels read it mixed (expectation mode)
int launch_noisy_wide(const NoiseArgs& a, int n, double* mix, hipStream_t st) {
    const double* hd = nullptr;
    if (a.diag && !a.shots && launch_readout_mix(a.diag, a.q, n, mix, st, &hd) != QHEA_OK) return QHEA_ELAUNCH;
    switch (n) {
        case 7: return launch_wide<7>(a, hd, st);
        case 8: return launch_wide<8>(a, hd, st);
        case 9: return launch_wide<9>(a, hd, st);
        case 10: return launch_wide<10>(a, hd, st);
        case 11: return launch_wide<11>(a, hd, st);
        case 12: return launch_wide<12>(a, hd, st);
        default: return QHEA_EUNSUPPORTED;
    }
}
constexpr TrajUnit kWideUnit{7, QHEA_MAX_QUBITS, true, 0};                   // qhea_model_forward_noisy is the path below 7

}  // namespace

int launch_readout_mix(const double* diag, double q, int n, double* mix, hipStream_t st, const double** hd) {
    hipLaunchKernelGGL(readout_mix_kernel, dim3(1), dim3(256), 0, st, diag, q, n, mix);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    *hd = mix + ((size_t)((n - 1) & 1) << n);
    return QHEA_OK;
}
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_noisy_wide_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise) {
    return traj_workspace_bytes(kWideUnit, desc, batch, noise);
}

int qhea_model_forward_noisy_wide(const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch,
                                  const double* trunk, const double* params, const double* ham_diag, const qhea_noise* noise,
                                  double* pred, double* stderr_out, void* workspace, size_t workspace_bytes, void* stream) {
    TrajCall t;
    const int rc = traj_open(kWideUnit, desc, row0, batch, branch, trunk, params, ham_diag, noise, pred, workspace, workspace_bytes,
                             stream, t);
    if (rc != QHEA_OK || t.c.empty) return rc;
    return traj_finish(t, launch_noisy_wide(t.a, t.c.mi.n, t.mix, t.c.st), pred, stderr_out);
}

}  // extern "C"
