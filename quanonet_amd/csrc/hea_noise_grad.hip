// hea_noise_grad.hip -- qhea_model_loss_grad_noisy_wide / qhea_model_train_steps_noisy_wide: the MSE loss of the sampled noisy
// forward (hea_noise_wide.hip, expectation mode) and its gradient with the random stream held fixed, n = 7..9.  The contract is
// stated in include/quanonet_hea.h; tests/noisy_traj_grad_reference.py restates the walk in numpy.
//
// For fixed draws a trajectory is an ideal circuit with fixed Pauli strings inserted, so its value v = sum_k p_k h'(k) is smooth
// in the angles and d v / d angle comes from the adjoint walk of bwd_kernel (hea_device.hpp) with the frames in it.
//
// noisy_grad_wave_kernel<N>: one wave per (row, tile of kGradTile trajectories), the state in Cfg<N>'s layout.  Per trajectory:
//   forward   the walk of noisy_wide_wave_kernel: RX per wire, the encoding frame; per sub-layer the n fused rotations, the ring,
//             the sub-layer frame; the same Philox words for the same (seed, global row, trajectory, location);
//   read-out  behind basis_change: v as the forward kernel adds it, lambda = h' psi (unweighted), both back through the dagger
//             of the basis change;
//   reverse   per sub-layer: the frame again on psi and lambda (X^x Z^z is its own inverse up to a sign that psi and lambda
//             share and every inner product takes twice), the reverse ring, per wire su2_inverse_with_inner; behind a block's
//             sub-layers its encoding frame, then per wire pauli_x_inner and RX^dagger.  The frames are recomputed from the
//             stream (one Philox call per lane and segment), not kept.
// Record form: the fused gate's (X, Y, Z) sums, as the ideal path records them -- one SU(2) inverse per wire on psi and on
// lambda, against three for a walk through RY RZ RY; noisy_grad_fold_kernel maps them to the three angles (the map is linear
// and depends on the parameters only, so it commutes with the sums over trajectories).
// Sums: a sub-layer's 3n inner products go over the wave by butterfly_sum, a block's n encoding ones by lane_reduce; the lane
// that ends up with a value adds it to the item's record in global memory -- the first trajectory of the tile stores, later
// ones read, add and store, the same lane every time, so program order is all the ordering there is.  No atomics.
// noisy_grad_fold_kernel: a row's tiles added in tile order and divided by T: pred (+ bias, as noisy_finish_kernel) and the
// record rec[E + 3 n blk][B] that launch_density_reduce (hea_density_grad.hip) reads; that launch does the weights, the
// frequency chain rule, grad[P], grad[P + 1] and Adam.  launch_noisy_grad_fold puts it behind hea_noise_grad_lds.hip's kernel
// (n = 10..12) too; what the two units share on the host is hea_noise_grad.hpp.
#include "hea_noise_grad.hpp"

namespace qhea {
namespace {

constexpr int kGradWaves = 4;               // waves per workgroup (independent; no LDS, no barrier)
// Trajectories per work item: part of the stated summation order.  A wave walks its trajectories one after another (0.24 ms
// each on the Q8 20 x 2 model), so at batch 100 a step lasts as long as one tile: measured there at T = 64,
// tiles of 64 / 32 / 16 / 8 / 4 take 15.1 / 7.6 / 3.8 / 1.9 / 1.5 ms, and at batch 2048 they are within 10 % of each other.  The
// price of a small tile is the workspace: one record of E + 3 n blk doubles per tile.
#ifndef QHEA_NOISE_GRAD_TILE
#define QHEA_NOISE_GRAD_TILE 4
#endif
constexpr int kGradTile = QHEA_NOISE_GRAD_TILE;
constexpr int kFoldThreads = 256;

// NoisyGradArgs, the workspace layout, the checks and the entry points' bodies: hea_noise_grad.hpp, shared with
// hea_noise_grad_lds.hip (n = 10..12)

template <int N>
__global__ __launch_bounds__(64 * kGradWaves) void noisy_grad_wave_kernel(NoisyGradArgs g) {
    using C = Cfg<N>;
    constexpr int R = C::R;
    const NoiseArgs& a = g.f;
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * kGradWaves + (threadIdx.x >> 6);
    if (item >= a.B * a.tiles) return;                                   // whole waves
    const long r = item / a.tiles, t0 = (item - r * a.tiles) * (long)kGradTile;
    const int tcount = (int)(a.T - t0 < kGradTile ? a.T - t0 : kGradTile);
    const unsigned long long row = (unsigned long long)(a.row0 + r);
    const double2* csr = a.cs + r * a.E;
    double* rec = g.items + item * (long)g.width;
    double* rec_w = rec + a.E;
    const int ring_fwd = ring_source<N>(lane, false), ring_rev = ring_source<N>(lane, true);
    const double off_term = g.hd ? 0.0 : a.off;

    double sum = 0.0, sq = 0.0;
    for (int tj = 0; tj < tcount; ++tj) {
        const unsigned traj = (unsigned)(t0 + tj);
        const bool first = tj == 0;
        double pr[R], pi[R], lr[R], li[R];
#pragma unroll
        for (int i = 0; i < R; ++i) { pr[i] = 0.0; pi[i] = 0.0; }
        pr[0] = lane == 0 ? 1.0 : 0.0;
        unsigned loc = 0;
        int s = 0, col = 0, x, z;
        for (int gi = 0; gi < 2; ++gi) {
            for (int b = 0; b < a.nb[gi]; ++b) {
                unsigned codes = segment_codes(a, loc, N, N, traj, row, lane);
                static_for<0, N>([&](auto q) {
                    constexpr int Q = decltype(q)::value;
                    const double2 c = csr[col + Q];
                    apply_rx<N, Q>(pr, pi, c.x, c.y);
                });
                enc_frame<N>(codes, loc, x, z);
                frame_regs<N>(pr, pi, x, z, lane);
                col += N; loc += N;
                for (int l = 0; l < a.ld[gi]; ++l, ++s, loc += 2 * N) {
                    codes = segment_codes(a, loc, 2 * N, N, traj, row, lane);
                    static_for<0, N>([&](auto q) {
                        constexpr int Q = decltype(q)::value;
                        constexpr bool kSigned = Q < C::LB && !kSwapQubit<N, Q>;   // the lane's variant of the gate table
                        const double4 v = a.gates[2 * (s * N + Q + N) + (kSigned ? (lane >> Q) & 1 : 0)];
                        apply_su2<N, Q>(pr, pi, v.x, v.y, v.z, v.w);
                    });
                    sub_frame<N>(codes, loc, x, z);
                    apply_ring<N, false>(pr, pi, lane, ring_fwd);
                    frame_regs<N>(pr, pi, x, z, lane);
                }
            }
        }
        // read-out: v as the forward kernel adds it, lambda = h' psi
        basis_change<N, false>(pr, pi, a.pauli, lane);
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const double hk = readout_weight<N>(a, g.hd, lane | (i << 6));
            v += (pr[i] * pr[i] + pi[i] * pi[i]) * hk;
            lr[i] = hk * pr[i]; li[i] = hk * pi[i];
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        v += off_term;
        sum += v; sq += v * v;
        if (a.pauli) {
            basis_change<N, true>(pr, pi, a.pauli, lane);
            basis_change<N, true>(lr, li, a.pauli, lane);
        }
        // reverse walk: blocks, sub-layers and wires in reverse order
        for (int gi = 1; gi >= 0; --gi) {
            for (int b = a.nb[gi] - 1; b >= 0; --b) {
                for (int l = a.ld[gi] - 1; l >= 0; --l) {
                    --s; loc -= 2 * N;
                    sub_frame<N>(segment_codes(a, loc, 2 * N, N, traj, row, lane), loc, x, z);
                    frame_regs<N>(pr, pi, x, z, lane);
                    frame_regs<N>(lr, li, x, z, lane);
                    apply_ring<N, true>(pr, pi, lane, ring_rev);
                    apply_ring<N, true>(lr, li, lane, ring_rev);
                    double acc3[C::KW];
#pragma unroll
                    for (int i = 0; i < C::KW; ++i) acc3[i] = 0.0;
                    static_rfor<0, N>([&](auto q) {
                        constexpr int Q = decltype(q)::value;
                        constexpr bool kSigned = Q < C::LB && !kSwapQubit<N, Q>;
                        const double4 u = a.gates[2 * (s * N + Q + N) + (kSigned ? (lane >> Q) & 1 : 0)];
                        su2_inverse_with_inner<N, Q>(pr, pi, lr, li, u, lane, acc3[3 * Q], acc3[3 * Q + 1], acc3[3 * Q + 2]);
                    });
                    const int vi = butterfly_sum<C::KW>(acc3, lane);
                    if (butterfly_owner<C::KW>(lane) && vi < 3 * N) {
                        double* p = rec_w + (long)s * 3 * N + vi;
                        *p = first ? acc3[0] : *p + acc3[0];
                    }
                }
                col -= N; loc -= N;
                enc_frame<N>(segment_codes(a, loc, N, N, traj, row, lane), loc, x, z);
                frame_regs<N>(pr, pi, x, z, lane);
                frame_regs<N>(lr, li, x, z, lane);
                double gx[C::KX];
#pragma unroll
                for (int i = 0; i < C::KX; ++i) gx[i] = 0.0;
                static_rfor<0, N>([&](auto q) {
                    constexpr int Q = decltype(q)::value;
                    const double2 c = csr[col + Q];
                    gx[Q] = pauli_x_inner<N, Q>(pr, pi, lr, li);
                    apply_rx<N, Q>(pr, pi, c.x, -c.y);
                    apply_rx<N, Q>(lr, li, c.x, -c.y);
                });
                lane_reduce<C::KX, C::LB>(gx, lane);                     // lane j < KX holds value j
                if (lane < N) {
                    double* p = rec + col + lane;
                    *p = first ? gx[0] : *p + gx[0];
                }
            }
        }
    }
    if (lane == 0) a.partial[item] = make_double2(sum, sq);
}

// One thread per value of a row: encoding column e, gate (s, q) or the row's pred.  Tiles in tile order, then / T; a gate's
// (X, Y, Z) become the derivatives of its angles a, b, c = w[s, 0..2, q] (reduce_xyz_block's map, hea_api.hip):
//   g_c = Y;  g_b = cos(c) Z + sin(c) X;  g_a = cos(b) Y - sin(b) cos(c) X + sin(b) sin(c) Z
__global__ __launch_bounds__(kFoldThreads) void noisy_grad_fold_kernel(NoisyGradArgs g, int n) {
    const NoiseArgs& a = g.f;
    const long r = blockIdx.y;
    const int u = blockIdx.x * kFoldThreads + threadIdx.x, ngates = n * g.blk;
    if (u > a.E + ngates) return;
    const double invT = 1.0 / (double)a.T;
    if (u == a.E + ngates) {                                             // noisy_finish_kernel's rule
        double S = 0.0;
        for (int t = 0; t < a.tiles; ++t) S += a.partial[r * a.tiles + t].x;
        const double p = S / (double)a.T + (a.bias ? a.bias[0] : 0.0);
        g.pred_ws[r] = p;
        if (g.pred) g.pred[r] = p;
        return;
    }
    const double* it = g.items + r * a.tiles * (long)g.width;
    if (u < a.E) {
        double S = 0.0;
        for (int t = 0; t < a.tiles; ++t) S += it[(long)t * g.width + u];
        g.rec[(long)u * a.B + r] = S * invT;
        return;
    }
    const int gq = u - a.E, s = gq / n, q = gq - s * n;
    const double* src = it + a.E + (long)s * 3 * n + 3 * q;
    double X = 0.0, Y = 0.0, Z = 0.0;
    for (int t = 0; t < a.tiles; ++t) {
        X += src[(long)t * g.width]; Y += src[(long)t * g.width + 1]; Z += src[(long)t * g.width + 2];
    }
    X *= invT; Y *= invT; Z *= invT;
    const double* ws = g.w + (long)s * 3 * n + q;
    double sb, cb, sc, cc;
    sincos(ws[n], &sb, &cb);
    sincos(ws[2 * n], &sc, &cc);
    double* out = g.rec + ((long)a.E + (long)s * 3 * n + q) * a.B + r;
    out[0] = cb * Y - sb * cc * X + sb * sc * Z;
    out[(long)n * a.B] = cc * Z + sc * X;
    out[(long)2 * n * a.B] = Y;
}

// one wave per (row, tile)
int launch_wave(int n, const NoisyGradArgs& g, hipStream_t st) {
    const long items = g.f.B * g.f.tiles;
    const dim3 grid((unsigned)((items + kGradWaves - 1) / kGradWaves)), block(64 * kGradWaves);
    switch (n) {
        case 7: hipLaunchKernelGGL(noisy_grad_wave_kernel<7>, grid, block, 0, st, g); break;
        case 8: hipLaunchKernelGGL(noisy_grad_wave_kernel<8>, grid, block, 0, st, g); break;
        case 9: hipLaunchKernelGGL(noisy_grad_wave_kernel<9>, grid, block, 0, st, g); break;
        default: return QHEA_EUNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}
constexpr GradUnit kWaveUnit{7, 9, kGradTile, launch_wave};

}  // namespace

int launch_noisy_grad_fold(const NoisyGradArgs& g, int n, int64_t batch, hipStream_t st) {
    const int units = g.f.E + n * g.blk + 1;
    hipLaunchKernelGGL(noisy_grad_fold_kernel, dim3((unsigned)((units + kFoldThreads - 1) / kFoldThreads), (unsigned)batch),
                       dim3(kFoldThreads), 0, st, g, n);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_noisy_wide_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise) {
    return wide_grad_workspace_bytes(kWaveUnit, desc, batch, noise);
}

int qhea_model_loss_grad_noisy_wide(const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch,
                                    const double* trunk, const double* y, const double* params, const double* ham_diag,
                                    const qhea_noise* noise, double inv_batch_total, double* grad, double* pred, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return wide_grad_loss_grad(kWaveUnit, desc, row0, batch, branch, trunk, y, params, ham_diag, noise, inv_batch_total, grad, pred,
                               workspace, workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_wide(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                      const double* branch, const double* trunk, const double* y, double* params,
                                      const double* ham_diag, const qhea_noise* noise, const double* inv_batch_total,
                                      double* grad, int64_t grad_stride, double* exp_avg, double* exp_avg_sq,
                                      int64_t first_step, double lr, double beta1, double beta2, double eps,
                                      double weight_decay, void* workspace, size_t workspace_bytes, void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return wide_grad_train_steps(kWaveUnit, desc, call, ham_diag, noise, lr);
}

}  // extern "C"
