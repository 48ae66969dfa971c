// hea_noise_device_wide.hip -- qhea_model_forward_noisy_device_wide: the quantum-jump trajectories of hea_noise_device.hip under
// the calibrated device noise model for n = 10..12, where the state lives in LDS.  Same quantity, same unravelling, same random
// stream (include/quanonet_hea.h); what differs is where the state lives and, with it, the order of the floating-point sums,
// which the header states.  tests/device_traj_wide_reference.py restates the formulation in numpy and
// tests/test_device_traj_wide_abi.py proves it against the gate-by-gate replay without a GPU.
//
// Layout: that of noisy_wide_lds_kernel (hea_noise_wide.hip).  One workgroup of 2^(n-4) threads per (row, tile of kTile
// trajectories) work item, the trajectories one after another, the state in LDS behind phys<4>, a gate layer in the three passes
// of hea_lds.hpp (16 amplitudes per thread and pass) with the ring folded into the last pass's scatter.
//
// Every relaxation site is a DIAGONAL operation on the 16 amplitudes a thread holds in a pass that exists anyway:
//   * Jumps go into the frame.  |0><1|_w = X_w Pi1_w: a fired jump zeroes the amplitudes whose wire w reads |0>, sets N2 = M and
//     toggles bit w of the frame's X mask; no exchange, no pass.  No jump scales the |1> half by sqrt(1 - gamma), N2 -= gamma M.
//     Dephasing toggles a Z bit.  The frame therefore depends on the jump decisions: every thread evolves it (the values are
//     workgroup-uniform and live in scalar registers), wave 0 cannot build it ahead of the layer as in hea_noise_wide.hip.
//   * The stored state keeps its pre-ring labels for the whole sub-layer.  Behind CNOT slot j the logical bit of a wire is a
//     parity of at most three stored index bits (ring_site_mask below), XORed with the frame's X bit of the wire: "reads |1>" is
//     parity(tp & m) ^ parity(J & (m >> A)) ^ x_w for local index J, the middle term a compile-time constant per J.
//   * ENC_q and ROT_q run inside the pass that holds qubit q in registers, right behind gate q; the 2 n ring sites run in the
//     last pass behind its rotations and before the scatter store, on the same registers.  The frame is pushed through each CNOT
//     (x_t ^= x_c, z_c ^= z_t) and applied by the store: an XOR of phys(x) on the store base, a sign from the pulled-back z.
// A site with gamma > 0 costs one masked sum over the thread's 16 |v|^2, one workgroup reduction and one select-scale; gamma = 0
// skips it by a scalar branch (a table entry), so the default setting runs the ideal circuit bit for bit.
//
// Choices:
//   * |v|^2 is recomputed at every site, not kept beside v: 16 more doubles would not fit beside the 64 of v and the gate.
//   * Every site has its own reduction; the TGT / CTL pair of a slot does not share one.  The summation order of a site is then
//     one rule for all four kinds of site.
//   * The butterfly is pair_sum (DPP and permlane swaps, hea_device.hpp), offsets 32 .. 1, as in hea_noise_device.hip.
// Reduction: the thread's masked terms in local-index order, the butterfly over the wave, then the waves in order through LDS
// slots.  n = 10 is one wave and needs no barrier; n = 11, 12 write one of two alternating slot sets, so a site costs ONE
// barrier: a wave can only reach the site after next -- which writes this set again -- through the next site's barrier, which
// every wave passes after it has read this one.  The wave-local relaxation between the first two passes (wave_local_passes,
// hea_lds.hpp) stays in the code but cannot hold where those passes contain sites with gamma > 0 at n = 11, 12: the site's
// reduction is a workgroup barrier anyway.
//
// Philox: lane c of wave 0 computes call c of the segment -- the n ENC calls of a block, or the 3 n calls of a sub-layer (ROT
// 0..n-1, then the ring's 2 n) -- and reduces it to a code (Pauli in bits 0..3, dephasing in bit 4) and the jump's word, as
// site_draws of hea_noise_device.hip; both go to LDS scratch in front of a barrier that opens the layer.  The per-call thresholds
// and per-site (gamma, sqrt(1 - gamma)) live in a table in the workspace (WideDevTable, 12 wires), filled by one prep launch and
// read by wave-uniform addresses where a site uses them.
//
// Shared, not this unit's: the table, the body of its prep kernel, site_pair, group_sum, jump_u, draw_code and the body of the
// entry point are hea_noise_jump.hpp's (with hea_noise_device.hip); ring_pull and the framed store of the last pass
// (store_framed) are hea_lds.hpp's (with hea_noise_wide.hip).  The ground-state fill, the basis-change gate, the cdf prefix and
// pick of the read-out and plain_layer are spelt out here and in hea_noise_wide.hip: every shared form tried changed the device
// code of a kernel (profiles/r27_device_code_identity.txt).
// The scratch, relax_site, segment_draws, jump_layer and plain_layer are hea_noise_jump_lds.hpp's, shared with the gradient unit
// hea_noise_device_grad_lds.hip; this kernel's device code did not change with the move (profiles/r32_device_code_identity.txt).
#include <climits>
#include <cmath>
#include <cstdint>

#include "hea_noise_jump_lds.hpp"

namespace qhea {
namespace {

template <int N>
__global__ __launch_bounds__((LCfg<N, kLG>::T)) void device_traj_lds_kernel(NoiseArgs a, const WideDevTable* __restrict__ tab,
                                                                            const double* __restrict__ hd) {
    constexpr int LG = kLG, M = 1 << LG;
    using L = LCfg<N, LG>;
    extern __shared__ __attribute__((aligned(16))) char jump_lds[];
    JumpScratch* sc = reinterpret_cast<JumpScratch*>(jump_lds);
    double2* psi = reinterpret_cast<double2*>(jump_lds + kScratchBytes);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long item = blockIdx.x;
    const WorkItem wi = work_item(a, item);
    Bases<N, LG> bs;
    bs.init(t);
    const double off_term = (a.shots || a.diag) ? 0.0 : a.off;
    NoRecord rec;

    double sum = 0.0, sq = 0.0;
    for (int tj = 0; tj < wi.tcount; ++tj) {
        const unsigned traj = (unsigned)(wi.t0 + tj);
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int p = t + j * L::T;
            psi[p] = make_double2(p == 0 ? 1.0 : 0.0, 0.0);              // |0..0>: phys(0) = 0
        }
        JumpState js{1.0, 0, 0, 0};
        unsigned call = 0;
        int s = 0, col = 0;
        for (int g = 0; g < 2; ++g) {
            for (int b = 0; b < a.nb[g]; ++b) {
                segment_draws(a, tab, sc, call, 0, N, N, traj, wi.row);  // its barrier also covers the initial state
                jump_layer<N, kEnc>(psi, bs, t, sc, tab, js, [&](int q) { return rx_su2(wi.csr[col + q]); }, rec);
                col += N; call += N;
                for (int l = 0; l < a.ld[g]; ++l, ++s) {
                    segment_draws(a, tab, sc, call, N, 3 * N, N, traj, wi.row);
                    jump_layer<N, kRot>(psi, bs, t, sc, tab, js, [&](int q) { return a.gates[2 * ((s + 1) * N + q)]; }, rec);
                    call += 3 * N;
                }
            }
        }
        if (a.pauli != QHEA_PAULI_Z) {                                   // same probabilities as H / H S^dagger
            constexpr double kR = 0.70710678118654752440;
            const double4 ub = a.pauli == QHEA_PAULI_X ? make_double4(kR, 0.0, kR, 0.0) : make_double4(kR, 0.0, 0.0, -kR);
            plain_layer<N>(psi, bs, [&](int) { return ub; });
        }
        if (a.shots && wave == 0) {
            // calls L .. L + 3: u, then per bit the flip words against both thresholds (the outcome picks the direction)
            const int j = lane & 3;
            const uint4 w = philox(make_uint4(a.L + (unsigned)j, traj, (unsigned)wi.row, (unsigned)(wi.row >> 32)), a.key0, a.key1);
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
            m01 = __shfl(m01, 0) | __shfl(m01, 1) | __shfl(m01, 2) | __shfl(m01, 3);
            m10 = __shfl(m10, 0) | __shfl(m10, 1) | __shfl(m10, 2) | __shfl(m10, 3);
            if (t == 0) { sc->m01 = m01; sc->m10 = m10; sc->u = unit_double(w.x, w.y); }
        }
        // thread t reads the 16 consecutive basis states 16 t .. 16 t + 15
        c2 v[M];
        load_group<N, 0, false, LG>(psi, bs.plain[0], v);
        double pk[M], part = 0.0;
#pragma unroll
        for (int j = 0; j < M; ++j) { pk[j] = v[j].x * v[j].x + v[j].y * v[j].y; part += pk[j]; }
        double val;
        if (!a.shots) {
            double num = 0.0;
#pragma unroll
            for (int j = 0; j < M; ++j) num += pk[j] * hd[(t << LG) | j];
            num = group_sum<6>(num);
            double tot = group_sum<6>(part);
            if constexpr (L::NW > 1) {
                if (lane == 0) { sc->rsum[0][wave] = num; sc->rsum[1][wave] = tot; }
                __syncthreads();
                num = sc->rsum[0][0]; tot = sc->rsum[1][0];
#pragma unroll
                for (int w = 1; w < L::NW; ++w) { num += sc->rsum[0][w]; tot += sc->rsum[1][w]; }
            }
            val = num / tot + off_term;
        } else {
            double c[M];
            c[0] = pk[0];
#pragma unroll
            for (int j = 1; j < M; ++j) c[j] = c[j - 1] + pk[j];
            const double inc = wave_scan(c[M - 1], lane);
            double before = __shfl_up(inc, 1);
            if (lane == 0) before = 0.0;
            double tot = group_sum<6>(part);
            if (lane == 63) sc->rsum[0][wave] = inc;
            if (lane == 0) sc->rsum[1][wave] = tot;
            __syncthreads();                                             // rsum, u, the flip masks
            double below = 0.0;
            for (int w = 0; w < wave; ++w) below += sc->rsum[0][w];
            below += before;
            if constexpr (L::NW > 1) {
                tot = sc->rsum[1][0];
#pragma unroll
                for (int w = 1; w < L::NW; ++w) tot += sc->rsum[1][w];
            }
            const double ut = sc->u * tot;
            int lo = INT_MAX, hi = -1;
#pragma unroll
            for (int j = M - 1; j >= 0; --j) {
                if (ut < below + c[j]) lo = (t << LG) | j;
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
            val = shot_value<N>(a.diag, a.off, a.co, out ^ ((out & sc->m10) | (~out & sc->m01 & (L::DIM - 1))));
        }
        sum += val; sq += val * val;
        __syncthreads();                                                 // psi and the scratch are rewritten
    }
    if (t == 0) a.partial[item] = make_double2(sum, sq);
}

// ---- prep: the table, and expectation mode's read-out weights ------------------------------------------------------------------

__global__ __launch_bounds__(256) void wide_tables_kernel(WideDevTable t, WideDevTable* __restrict__ out,
                                                          const double* __restrict__ diag, double co, int n,
                                                          double* __restrict__ buf) {
    jump_tables_body(t, out, diag, co, n, buf);
}

template <int N>
int launch_traj_lds(const NoiseArgs& a, const WideDevTable* tab, const double* hd, hipStream_t st) {
    using L = LCfg<N, kLG>;
    constexpr size_t smem = kScratchBytes + L::STATE_BYTES;
    return launch_dynamic_lds(device_traj_lds_kernel<N>, dim3((unsigned)(a.B * a.tiles)), dim3(L::T), smem, st, a, tab, hd);
}

int launch_device_traj_wide(const NoiseArgs& a, int n, const WideDevTable* tab, const double* hd, hipStream_t st) {
    switch (n) {
        case 10: return launch_traj_lds<10>(a, tab, hd, st);
        case 11: return launch_traj_lds<11>(a, tab, hd, st);
        case 12: return launch_traj_lds<12>(a, tab, hd, st);
        default: return QHEA_EUNSUPPORTED;
    }
}

// the uniform units' layout with the read-out region of the wide ones, then the table
constexpr TrajUnit kJumpWideUnit{10, QHEA_MAX_QUBITS, true, sizeof(WideDevTable)};

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_noisy_device_wide_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling) {
    return jump_workspace_bytes(kJumpWideUnit, desc, batch, sampling);
}

int qhea_model_forward_noisy_device_wide(const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch,
                                         const double* trunk, const double* params, const double* ham_diag,
                                         const qhea_device_noise* dn, const qhea_sampling* sampling, double* pred,
                                         double* stderr_out, void* workspace, size_t workspace_bytes, void* stream) {
    return jump_forward(kJumpWideUnit, wide_tables_kernel, launch_device_traj_wide, desc, row0, batch, branch, trunk, params,
                        ham_diag, dn, sampling, pred, stderr_out, workspace, workspace_bytes, stream);
}

}  // extern "C"
