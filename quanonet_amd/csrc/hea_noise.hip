// hea_noise.hip -- qhea_model_forward_noisy: the model forward under depolarizing gate noise and readout error, estimated from
// Monte-Carlo trajectories (expectation mode) or sampled shots (shot mode).  Noise model, random-number layout and estimators are
// the contract stated in include/quanonet_hea.h; tests/noise_oracle.py replays them gate by gate.
//
// Layout: one amplitude per lane, n = 2..6; a wave holds 64 / 2^n (row, trajectory) slots of one row.  A work item is one wave
// and kTile consecutive trajectories of one row; slot j runs trajectories j, j + slots, ... of the tile and keeps its (sum, sum of
// squares) in trajectory order; the slots' sums are added in slot order into the item's partial, and the finish kernel adds a
// row's items in tile order.  Every summation order therefore depends on n and the trajectory count only -- not on the batch,
// the chunking or the grid -- and no floating-point atomics are used.
//
// Gates come from prep_model_kernel's tables (hea_model.hpp): the fused RY RZ RY gate per wire and sub-layer, and (cos, sin) of
// every encoding angle per row; RX is applied on its own because noise sits between it and the first rotation.  Sampled Paulis
// are kept as an X mask and a Z mask (a Pauli string up to a global phase) and pushed through the CNOTs of the ring by Clifford
// conjugation, so that a sub-layer's ring stays one lane gather followed by at most one gather for the whole sub-layer's errors
// (skipped when no slot of the wave drew one).  Philox calls are shared by the lanes of a slot: at each segment (the encoding of
// a block, or one sub-layer) lane k of the slot computes the segment's call k and turns its four words into the error codes of
// its two locations; every location then reads its code from that lane.
//
// The stream, the frame (apply_frame) and u of the cdf search are hea_noise_traj.hpp's, shared with hea_noise_wide.hip and
// hea_noise_device.hip.  Where the kernel below still spells out what those units also hold, the shared form changed its device
// code (profiles/r25_device_code_identity.txt).
#include <cmath>
#include <cstdint>

#include "hea_noise_traj.hpp"

namespace qhea {
namespace {

constexpr int kNoiseWaves = 4;              // waves per workgroup (independent; no LDS, no barrier)

template <int N>
__global__ __launch_bounds__(64 * kNoiseWaves) void noisy_fwd_kernel(NoiseArgs a) {
    constexpr int D = 1 << N, SL = 64 / D;
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * kNoiseWaves + (threadIdx.x >> 6);
    if (item >= a.B * a.tiles) return;                                   // whole waves
    // (written out, not work_item(): with it this kernel's device code changes)
    const long r = item / a.tiles;
    const long t0 = (item - r * a.tiles) * (long)kTile;
    const int tcount = (int)(a.T - t0 < kTile ? a.T - t0 : kTile);
    const int k = lane & (D - 1), base = lane - k, slot = lane / D;
    const unsigned long long row = (unsigned long long)(a.row0 + r);
    const double2* csr = a.cs + r * a.E;

    int ring = k;                                                        // the ring CNOT(1->0) ... CNOT(0->n-1) as one gather
#pragma unroll
    for (int j = N - 1; j >= 0; --j) ring ^= ((ring >> ((j + 1) % N)) & 1) << j;

    // expectation mode: value = off_term + sum_k p_k h(k), readout error folded in
    double h = 0.0, off_term = 0.0;
    if (!a.shots) {
        if (a.diag) {
            for (int j = 0; j < D; ++j) {
                double w = 1.0;
                for (int i = 0; i < N; ++i) w *= ((j ^ k) >> i) & 1 ? a.q : 1.0 - a.q;
                h += w * a.diag[j];
            }
        } else {
            h = a.co * (1.0 - 2.0 * a.q) * (double)(N - 2 * (int)__popc(k));
            off_term = a.off;
        }
    }

    double sum = 0.0, sq = 0.0;
    for (int it = 0; it < tcount; it += SL) {
        const int tj = it + slot;
        const unsigned traj = (unsigned)(t0 + tj);
        double re = k == 0 ? 1.0 : 0.0, im = 0.0;
        unsigned loc = 0;
        int s = 0, col = 0;
        for (int g = 0; g < 2; ++g) {
            for (int b = 0; b < a.nb[g]; ++b) {
                // encoding RX on every wire, then one-qubit depolarizing noise on every wire
                unsigned codes = segment_codes(a, loc, N, N, traj, row, k);
                int x = 0, z = 0;
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    const double2 c = csr[col + q];
                    const double pr = __shfl(re, lane ^ (1 << q)), pi = __shfl(im, lane ^ (1 << q));
                    const double nr = c.x * re + c.y * pi, ni = c.x * im - c.y * pr;
                    re = nr; im = ni;
                    const unsigned p = code_at(codes, loc, loc + q, base);
                    x |= pauli_x(p, q); z |= pauli_z(p, q);
                }
                apply_frame(re, im, x, z, k, base);
                col += N; loc += N;
                for (int l = 0; l < a.ld[g]; ++l, ++s, loc += 2 * N) {
                    codes = segment_codes(a, loc, 2 * N, N, traj, row, k);
                    x = 0; z = 0;
#pragma unroll
                    for (int q = 0; q < N; ++q) {                        // fused RY RZ RY per wire, then its noise
                        const double4 v = a.gates[2 * (s * N + q + N) + ((k >> q) & 1)];
                        const double pr = __shfl(re, lane ^ (1 << q)), pi = __shfl(im, lane ^ (1 << q));
                        const double nr = v.x * re - v.y * im + v.z * pr - v.w * pi;
                        const double ni = v.x * im + v.y * re + v.z * pi + v.w * pr;
                        re = nr; im = ni;
                        const unsigned p = code_at(codes, loc, loc + q, base);
                        x |= pauli_x(p, q); z |= pauli_z(p, q);
                    }
#pragma unroll
                    for (int j = 0; j < N; ++j) {                        // CNOT(c -> t) conjugates the frame, then its own noise
                        const int c = (j + 1) % N, t = j;
                        x ^= ((x >> c) & 1) << t;
                        z ^= ((z >> t) & 1) << c;
                        const unsigned p = code_at(codes, loc, loc + N + j, base);
                        x ^= pauli_x(p >> 2, c) | pauli_x(p & 3u, t);
                        z ^= pauli_z(p >> 2, c) | pauli_z(p & 3u, t);
                    }
                    const double pr = __shfl(re, base + ring), pi = __shfl(im, base + ring);
                    re = pr; im = pi;
                    apply_frame(re, im, x, z, k, base);
                }
            }
        }
        // noiseless basis change of the X / Y read-outs: H, or H S^dagger, on every wire
        if (a.pauli != QHEA_PAULI_Z) {
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const int bit = (k >> q) & 1;
                if (a.pauli == QHEA_PAULI_Y && bit) { const double t = re; re = im; im = -t; }
                const double pr = __shfl(re, lane ^ (1 << q)), pi = __shfl(im, lane ^ (1 << q));
                re = M_SQRT1_2 * (bit ? pr - re : re + pr);
                im = M_SQRT1_2 * (bit ? pi - im : im + pi);
            }
        }
        const double pk = re * re + im * im;
        double v;
        if (!a.shots) {
            v = pk * h;
#pragma unroll
            for (int o = D / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
            v += off_term;
        } else {
            // one measured bitstring: u against the cdf in index order, then n readout flips
            const unsigned cm = (a.L + 1) >> 1;
            const uint4 w0 = philox(make_uint4(cm, traj, (unsigned)row, (unsigned)(row >> 32)), a.key0, a.key1);
            const uint4 w1 = philox(make_uint4(cm + 1, traj, (unsigned)row, (unsigned)(row >> 32)), a.key0, a.key1);
            const double u = unit_double(w0.x, w0.y);
            double acc = 0.0;
            int out = -1, last = 0;
            for (int j = 0; j < D; ++j) {
                const double pj = __shfl(pk, base + j);
                acc += pj;
                if (out < 0 && u < acc) out = j;
                if (pj > 0.0) last = j;
            }
            if (out < 0) out = last;
            const unsigned rw[6] = {w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
            for (int i = 0; i < N; ++i) out ^= (unsigned long long)rw[i] < a.thrq ? 1 << i : 0;
            // (written out, not shot_value<N>: this kernel is built without that function's contraction pragma)
            v = a.diag ? a.diag[out] : a.off + a.co * (double)(N - 2 * (int)__popc(out));
        }
        if (tj < tcount) { sum += v; sq += v * v; }
    }
    double S = 0.0, Q = 0.0;
#pragma unroll
    for (int j = 0; j < SL; ++j) { S += __shfl(sum, j * D); Q += __shfl(sq, j * D); }
    if (lane == 0) a.partial[item] = make_double2(S, Q);
}

// row r: mean over its T values (+ bias), standard error = sample standard deviation / sqrt(T) (0 for T = 1)
__global__ __launch_bounds__(256) void noisy_finish_kernel(const double2* __restrict__ partial, int tiles, long B, long T,
                                                           const double* __restrict__ bias, double* __restrict__ pred,
                                                           double* __restrict__ se) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    double S = 0.0, Q = 0.0;
    for (int t = 0; t < tiles; ++t) {
        const double2 v = partial[r * tiles + t];
        S += v.x; Q += v.y;
    }
    const double mean = S / (double)T;
    pred[r] = mean + (bias ? bias[0] : 0.0);
    if (se) {
        const double var = T > 1 ? (Q - S * mean) / (double)(T - 1) : 0.0;
        se[r] = var > 0.0 ? sqrt(var / (double)T) : 0.0;
    }
}

int launch_noisy(const NoiseArgs& a, int n, hipStream_t st) {
    const long items = a.B * a.tiles;
    const dim3 grid((unsigned)((items + kNoiseWaves - 1) / kNoiseWaves)), block(64 * kNoiseWaves);
    switch (n) {
        case 2: hipLaunchKernelGGL(noisy_fwd_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(noisy_fwd_kernel<3>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(noisy_fwd_kernel<4>, grid, block, 0, st, a); break;
        case 5: hipLaunchKernelGGL(noisy_fwd_kernel<5>, grid, block, 0, st, a); break;
        case 6: hipLaunchKernelGGL(noisy_fwd_kernel<6>, grid, block, 0, st, a); break;
        default: return QHEA_EUNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}
constexpr TrajUnit kLaneUnit{QHEA_MIN_QUBITS, 6, false, 0};                 // lane-resident states only

}  // namespace

int launch_noisy_finish(const double2* partial, int tiles, int64_t B, int64_t T, const double* bias, double* pred, double* se,
                        hipStream_t st) {
    hipLaunchKernelGGL(noisy_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, partial, tiles, (long)B, (long)T,
                       bias, pred, se);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_noisy_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise) {
    return traj_workspace_bytes(kLaneUnit, desc, batch, noise);
}

int qhea_model_forward_noisy(const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch, const double* trunk,
                             const double* params, const double* ham_diag, const qhea_noise* noise, double* pred,
                             double* stderr_out, void* workspace, size_t workspace_bytes, void* stream) {
    TrajCall t;
    const int rc = traj_open(kLaneUnit, desc, row0, batch, branch, trunk, params, ham_diag, noise, pred, workspace, workspace_bytes,
                             stream, t);
    if (rc != QHEA_OK || t.c.empty) return rc;
    return traj_finish(t, launch_noisy(t.a, t.c.mi.n, t.c.st), pred, stderr_out);
}

}  // extern "C"
