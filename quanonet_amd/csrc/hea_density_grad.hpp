// hea_density_grad.hpp -- the reverse walk through the density matrix that the gradient units share (hea_density_grad.hip:
// the uniform channels of qhea_noise; hea_density_device_grad.hip: the channel sites of qhea_device_noise; hea_density_wide_grad.hip: the uniform channels on the
// tiles of n = 7..9; hea_density_device_wide_grad.hip: the channel sites on those tiles): the two compiler
// pins, a thread's share of a trace, the un-rotations, the reverse of the CNOT with its two-qubit channel, the row context with
// the sum of a pass' traces over the row, the read-out basis passes, the workspace layout and the reduce launch.  The device
// code sits in an unnamed namespace like hea_density.hpp's: each unit compiles its own copy into its own kernels.  Host side:
// the backward launcher and the one body of the units' entry points (grad_loss_grad, grad_train_steps over a unit record).
#pragma once
#include "hea_density.hpp"
#include "hea_adam.hpp"
#include "hea_sincos.hpp"

namespace qhea {

// reduce_density_kernel (hea_density_grad.hip) on `st`: the rows of rec[E + 3 n blk][B] added per parameter in a fixed order
// with weight 2 (pred - y) inv_bt, the frequency chain rule, sum (pred - y)^2 and sum y^2 into grad[P + 2], and with adam.p
// the Adam update of hea_adam.hpp
int launch_density_reduce(const qhea_model_desc* desc, const ModelInfo& mi, int64_t batch, const double* branch,
                          const double* trunk, const double* y, const double* rec, const double* pred, double inv_bt,
                          double* grad, const AdamArgs& adam, hipStream_t st);

namespace {

constexpr int kTracesPerPass = 8;                                        // two wires x (three angles + the encoding)
// Threads of a density_bwd_kernel workgroup: a row's 4^(n-2) threads, at least QHEA_DENS_BWD_THREADS.  A workgroup's rows are
// independent (they meet only at the pass barriers), so the choice changes no result; it decides how many CUs a small batch
// spreads over and how many rows share a CU's LDS.  Measured at 64 and 256: one wave per workgroup is faster
// at every batch measured (n = 5, batch 100: 1.55 against 1.93 ms per step), so that is what is built.
#ifndef QHEA_DENS_BWD_THREADS
#define QHEA_DENS_BWD_THREADS 64
#endif
template <int N> constexpr int bwd_threads() {
    return (1 << (2 * N - 4)) > QHEA_DENS_BWD_THREADS ? (1 << (2 * N - 4)) : QHEA_DENS_BWD_THREADS;
}

// LDS of a backward workgroup: rho and O of its rows, h'[D], and two buffers of the waves' trace partials (n = 6)
template <int N> constexpr size_t bwd_lds_bytes() {
    constexpr int TPR = 1 << (2 * N - 4), RPW = bwd_threads<N>() / TPR, WPR = TPR > 64 ? TPR / 64 : 1;
    return 2 * (size_t)RPW * (1 << (2 * N)) * sizeof(double2) + (1 << N) * sizeof(double) + 2 * WPR * kTracesPerPass * sizeof(double);
}

// A pass' 32 LDS addresses depend on the thread alone, so the compiler computes those of every pass once, ahead of the loop
// over the sub-layers, and keeps 32 n values alive through it (up to 198 AGPRs at n = 6, beside the 256 VGPRs the elements and
// their arithmetic take).  A zero it cannot see through, taken inside the pass, makes it form them where they are used.
__device__ __forceinline__ int opaque_zero() {
    int z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return z;
}

// A trace is needed only when the pass ends, and the compiler would move its arithmetic down to there -- keeping the 32 elements
// it reads alive past the un-rotation that replaces them, once per trace.  This pins the value where it is computed.
__device__ __forceinline__ double pinned(double t) {
    asm volatile("" : "+v"(t));
    return t;
}

__device__ __forceinline__ double im_cj(double2 a, double2 b) { return a.x * b.y - a.y * b.x; }     // Im(conj(a) b)
__device__ __forceinline__ double re_cj(double2 a, double2 b) { return a.x * b.x + a.y * b.y; }     // Re(conj(a) b)

// this thread's share of Im Tr(O sigma_AX rho) for the wire of stride S (AX: 0 X, 1 Y, 2 Z)
template <int S, int AX>
__device__ __forceinline__ double trace16(const double2 (&o)[16], const double2 (&e)[16]) {
    double t = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int b = S == 1 ? 4 * m : m;
#pragma unroll
        for (int c = 0; c < 2; ++c) {                                    // column bit; elements (row bit 0, row bit 1)
            const double2 o0 = o[b + S * (2 * c)], o1 = o[b + S * (2 * c + 1)];
            const double2 r0 = e[b + S * (2 * c)], r1 = e[b + S * (2 * c + 1)];
            if (AX == 0) t += im_cj(o0, r1) + im_cj(o1, r0);
            else if (AX == 1) t += re_cj(o1, r0) - re_cj(o0, r1);
            else t += im_cj(o0, r0) - im_cj(o1, r1);
        }
    }
    return t;
}

// e <- R e R^T with R = RY(theta)^dagger = [[c, s], [-s, c]]
template <int S>
__device__ __forceinline__ void unrotate_y(double2 (&e)[16], double c, double s) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int b = S == 1 ? 4 * m : m;
        const double2 x00 = e[b], x10 = e[b + S], x01 = e[b + 2 * S], x11 = e[b + 3 * S];
        const double2 r00 = make_double2(c * x00.x + s * x10.x, c * x00.y + s * x10.y);
        const double2 r10 = make_double2(c * x10.x - s * x00.x, c * x10.y - s * x00.y);
        const double2 r01 = make_double2(c * x01.x + s * x11.x, c * x01.y + s * x11.y);
        const double2 r11 = make_double2(c * x11.x - s * x01.x, c * x11.y - s * x01.y);
        e[b] = make_double2(c * r00.x + s * r01.x, c * r00.y + s * r01.y);
        e[b + 2 * S] = make_double2(c * r01.x - s * r00.x, c * r01.y - s * r00.y);
        e[b + S] = make_double2(c * r10.x + s * r11.x, c * r10.y + s * r11.y);
        e[b + 3 * S] = make_double2(c * r11.x - s * r10.x, c * r11.y - s * r10.y);
    }
}

// e <- U e U^dagger with U = RX(theta)^dagger = [[c, i s], [i s, c]]
template <int S>
__device__ __forceinline__ void unrotate_x(double2 (&e)[16], double c, double s) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int b = S == 1 ? 4 * m : m;
        const double2 x00 = e[b], x10 = e[b + S], x01 = e[b + 2 * S], x11 = e[b + 3 * S];
        // U on the row index: i s (x + i y) = (-s y, s x)
        const double2 r00 = make_double2(c * x00.x - s * x10.y, c * x00.y + s * x10.x);
        const double2 r10 = make_double2(c * x10.x - s * x00.y, c * x10.y + s * x00.x);
        const double2 r01 = make_double2(c * x01.x - s * x11.y, c * x01.y + s * x11.x);
        const double2 r11 = make_double2(c * x11.x - s * x01.y, c * x11.y + s * x01.x);
        // U* on the column index: -i s (x + i y) = (s y, -s x)
        e[b] = make_double2(c * r00.x + s * r01.y, c * r00.y - s * r01.x);
        e[b + 2 * S] = make_double2(c * r01.x + s * r00.y, c * r01.y - s * r00.x);
        e[b + S] = make_double2(c * r10.x + s * r11.y, c * r10.y - s * r11.x);
        e[b + 3 * S] = make_double2(c * r11.x + s * r10.y, c * r11.y - s * r10.x);
    }
}

// e <- D e D^dagger with D = RZ(theta)^dagger: rho10 *= exp(-i theta), rho01 *= exp(i theta); (c, s) = (cos, sin)(theta / 2)
template <int S>
__device__ __forceinline__ void unrotate_z(double2 (&e)[16], double c, double s) {
    const double C = c * c - s * s, Sn = 2.0 * s * c;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int b = S == 1 ? 4 * m : m;
        const double2 x10 = e[b + S], x01 = e[b + 2 * S];
        e[b + S] = make_double2(C * x10.x + Sn * x10.y, C * x10.y - Sn * x10.x);
        e[b + 2 * S] = make_double2(C * x01.x - Sn * x01.y, C * x01.y + Sn * x01.x);
    }
}

// The fused rotation of wire q in sub-layer s in reverse, behind the unit's own channel: for RY(w2), RZ(w1), RY(w0) in turn the
// trace, then the un-rotation of rho and O.  tr[k] = this thread's share of d pred / d w[s, k, q]; tr[3] (the encoding's) = 0.
template <int N, int S>
__device__ __forceinline__ void undo_rotations(double2 (&e)[16], double2 (&o)[16], const double* w, int s, int q, double* tr) {
    const double* ws = w + (long)s * 3 * N + q;
    double sn, cn;
    tr[2] = pinned(trace16<S, 1>(o, e));
    fast_sincos(0.5 * ws[2 * N], &sn, &cn);
    unrotate_y<S>(e, cn, sn);
    unrotate_y<S>(o, cn, sn);
    tr[1] = pinned(trace16<S, 2>(o, e));
    fast_sincos(0.5 * ws[N], &sn, &cn);
    unrotate_z<S>(e, cn, sn); unrotate_z<S>(o, cn, sn);
    tr[0] = pinned(trace16<S, 1>(o, e));
    fast_sincos(0.5 * ws[0], &sn, &cn);
    unrotate_y<S>(e, cn, sn);
    unrotate_y<S>(o, cn, sn);
    tr[3] = 0.0;
}

// channel (inverse on rho), then CNOT(c -> t) on both indices: the reverse of cnot_depolarize2
__device__ __forceinline__ void undo_cnot2(double2 (&e)[16], double keep, double mix) {
    const double sx = (e[0].x + e[3].x) + (e[12].x + e[15].x), sy = (e[0].y + e[3].y) + (e[12].y + e[15].y);
    double2 r[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool eq = k == 0 || k == 3 || k == 12 || k == 15;
        r[k].x = eq ? keep * e[k].x + mix * sx : keep * e[k].x;
        r[k].y = eq ? keep * e[k].y + mix * sy : keep * e[k].y;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) e[k] = r[k ^ ((k >> 2) & 1) ^ (((k >> 3) & 1) << 1)];
}

// The argument record and the wire pieces of the uniform channels (hea_density_grad.hip, hea_density_wide_grad.hip)
struct DensGradArgs {
    DensArgs f;                             // the forward's arguments (f.pred: the caller's pred or NULL; f.sd = NULL)
    const double* w;                        // ansatz angles [blk, 3, n]
    double o1_keep, o1_mix, o1_off;         // one-qubit channel on O (the forward's) ...
    double r1_keep, r1_mix, r1_off;         // ... and its inverse on rho
    double o2_keep, o2_mix, r2_keep, r2_mix;
    double* pred_ws;                        // [B]
    double* rec;                            // [E + 3 n blk][B]: d pred_b / d x[b, e], then d pred_b / d w[s, k, q]
};

// one-qubit channel with given coefficients (the forward's on O, the inverse's on rho)
template <int S>
__device__ __forceinline__ void channel1(double2 (&e)[16], double keep, double mix, double off) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int b = S == 1 ? 4 * m : m;
        const double2 d0 = e[b], d1 = e[b + 3 * S];
        e[b] = make_double2(keep * d0.x + mix * d1.x, keep * d0.y + mix * d1.y);
        e[b + 3 * S] = make_double2(keep * d1.x + mix * d0.x, keep * d1.y + mix * d0.y);
        e[b + S].x *= off; e[b + S].y *= off;
        e[b + 2 * S].x *= off; e[b + 2 * S].y *= off;
    }
}

// encoding of wire q: channel, trace (slot 3 of the wire's four), RX^dagger
template <int S>
__device__ __forceinline__ void undo_encoding(double2 (&e)[16], double2 (&o)[16], const DensGradArgs& a, double2 c, double* tr) {
    channel1<S>(e, a.r1_keep, a.r1_mix, a.r1_off);
    channel1<S>(o, a.o1_keep, a.o1_mix, a.o1_off);
    tr[3] = pinned(trace16<S, 0>(o, e));
    unrotate_x<S>(e, c.x, c.y);
    unrotate_x<S>(o, c.x, c.y);
}

// wire q's gates of sub-layer s in reverse; tr[k] = this thread's share of d pred / d w[s, k, q], tr[3] of d pred / d x[col + q]
template <int N, int S>
__device__ __forceinline__ void undo_wire(double2 (&e)[16], double2 (&o)[16], const DensGradArgs& a, const double2* csr, int s,
                                          int col, bool enc, int q, double* tr) {
    channel1<S>(e, a.r1_keep, a.r1_mix, a.r1_off);
    channel1<S>(o, a.o1_keep, a.o1_mix, a.o1_off);
    undo_rotations<N, S>(e, o, a.w, s, q, tr);
    if (enc) undo_encoding<S>(e, o, a, csr[col + q], tr);
}

// What the passes need of the workgroup: the row's rho and O, its rank and fold, where its record goes
template <int N> struct RowCtx {
    static constexpr int TPR = 1 << (2 * N - 4), WPR = TPR > 64 ? TPR / 64 : 1;
    double2* rho; double2* obs;
    double* red;                            // [2][WPR][kTracesPerPass], n = 6 only
    int rank, sf, parity;
    long r, B;
    bool live;
};

// Adds tr[0 .. 8) over the row's threads and stores the sums whose record index idx[i] is >= 0 (to a.rec[idx[i]][row]).  Called by every thread of the
// workgroup after a reverse pass has stored its elements, with the pass' closing barrier inside.
template <int N, class Args>
__device__ __forceinline__ void flush_traces(RowCtx<N>& cx, const Args& a, double (&tr)[kTracesPerPass],
                                             const int (&idx)[kTracesPerPass]) {
    using C = RowCtx<N>;
    constexpr int W = C::TPR < 64 ? C::TPR : 64;
#pragma unroll
    for (int i = 0; i < kTracesPerPass; ++i) {
#pragma unroll
        for (int o = W / 2; o >= 1; o >>= 1) tr[i] += __shfl_xor(tr[i], o);
    }
    if constexpr (C::WPR == 1) {
        __syncthreads();
        if (cx.rank == 0 && cx.live) {
#pragma unroll
            for (int i = 0; i < kTracesPerPass; ++i)
                if (idx[i] >= 0) a.rec[(long)idx[i] * cx.B + cx.r] = tr[i];
        }
    } else {
        double* red = cx.red + cx.parity * (C::WPR * kTracesPerPass);
        const int tid = (int)threadIdx.x;
        if ((tid & 63) == 0) {
#pragma unroll
            for (int i = 0; i < kTracesPerPass; ++i) red[(tid >> 6) * kTracesPerPass + i] = tr[i];
        }
        __syncthreads();
        if (tid < kTracesPerPass && cx.live) {
            int my = -1;
#pragma unroll
            for (int i = 0; i < kTracesPerPass; ++i) my = tid == i ? idx[i] : my;
            if (my >= 0) {
                double t = red[tid];
                for (int wv = 1; wv < C::WPR; ++wv) t += red[wv * kTracesPerPass + tid];
                a.rec[(long)my * cx.B + cx.r] = t;
            }
        }
        cx.parity ^= 1;                                                  // the next pass' partials go to the other buffer
    }
}

// U on every wire of one matrix in LDS (no noise): KIND 3 = H, 4 = S H (the daggers of the read-out basis changes)
template <int N, int J, int KIND>
__device__ __forceinline__ void basis_passes_back(double2* row, int rank, int sf) {
    if constexpr (J < N) {
        using P = Pass<N, J>;
        const int i0 = P::base(rank | opaque_zero()), b = i0 ^ fold(i0) ^ sf;
        double2 e[16];
        P::load(e, row, b);
        const U2 h = KIND == 3 ? U2{{M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {-M_SQRT1_2, 0.0}}
                               : U2{{M_SQRT1_2, 0.0}, {M_SQRT1_2, 0.0}, {0.0, M_SQRT1_2}, {0.0, -M_SQRT1_2}};
        apply_gate<1>(e, h);
        if (J + 1 < N) apply_gate<4>(e, h);
        P::store(e, row, b);
        __syncthreads();
        basis_passes_back<N, J + 2, KIND>(row, rank, sf);
    }
}

struct DensGradLayout { size_t off_gates, off_cs, off_pred, off_rec, total; };

DensGradLayout dens_grad_layout(const ModelInfo& mi, int64_t B) {
    DensGradLayout L{};
    const DensLayout F = dens_layout(mi, B);
    L.off_gates = F.off_gates; L.off_cs = F.off_cs;
    size_t p = F.total;
    L.off_pred = p; p = align256(p + (size_t)B * sizeof(double));
    L.off_rec = p;  p = align256(p + (size_t)B * ((size_t)mi.sh.E + (size_t)3 * mi.n * mi.sh.blk) * sizeof(double));
    L.total = p;
    return L;
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// a backward kernel (density_bwd_kernel<N>, density_dev_bwd_kernel<N>) over B rows
template <int N, class Args>
int launch_density_bwd(void (*kernel)(Args), long B, const Args& a, hipStream_t st) {
    constexpr int T = bwd_threads<N>(), RPW = T / (1 << (2 * N - 4));
    return launch_dynamic_lds(kernel, dim3((unsigned)((B + RPW - 1) / RPW)), dim3(T), bwd_lds_bytes<N>(), st, a);
}

// One batch of a gradient call as a unit's backward launch sees it: the checked call, the prep tables and the regions of the
// workspace (laid out for `batch` rows; bmax: the rows the call's workspace was sized for)
struct GradBatch {
    const qhea_model_desc* desc; const ModelInfo& mi;
    const double* params; const double* ham_diag;
    int64_t batch, bmax;
    const double4* gates; const double2* cs;
    double* pred;                           // the caller's pred or NULL
    double* pred_ws; double* rec;
    char* ws; hipStream_t st;
};

// the argument record of the uniform channels for one batch: the forward's arguments, the channels on O and their inverses on rho
DensGradArgs dens_grad_args(const GradBatch& b, const qhea_noise* noise) {
    DensGradArgs a{};
    a.f = dens_args(b.desc, b.mi, noise, b.params, b.ham_diag, b.batch, b.gates, b.cs);
    a.f.pred = b.pred; a.f.sd = nullptr;
    a.w = b.params + b.mi.off_ans;
    a.o1_keep = a.f.d1_keep; a.o1_mix = a.f.d1_mix; a.o1_off = a.f.d1_off;
    a.r1_off = 1.0 / a.f.d1_off; a.r1_keep = a.f.d1_keep * a.r1_off; a.r1_mix = -a.f.d1_mix * a.r1_off;
    a.o2_keep = a.f.d2_keep; a.o2_mix = a.f.d2_mix;
    a.r2_keep = 1.0 / a.f.d2_keep; a.r2_mix = -a.f.d2_mix * a.r2_keep;
    a.pred_ws = b.pred_ws; a.rec = b.rec;
    return a;
}

// The body of the gradient units' entry points.  A unit record U (DensGradUnit of hea_density_grad.hip, DevGradUnit of
// hea_density_device_grad.hip, WideGradUnit and DevWideGradUnit of the two tiled units) gives
//   Noise                              the call's noise setting (qhea_noise, qhea_device_noise)
//   kStepCheckFirst                    where train_steps reports first_step < 1: true: with the descriptor and n_steps < 0, ahead
//                                      of every other check; false: after U::check and before the return of a call without steps
//   workspace_bytes(mi, B)             the call's workspace for B rows
//   check(desc, ham_diag, noise, count, trunk, required, workspace, stream, c)      what opens the call
//   batch_ok(mi, B)                    whether the unit's grids reach B rows (QHEA_EINVAL otherwise, ahead of the workspace check)
//   once(mi, noise, ws, bmax, st)      what is launched once per call, or nothing
//   launch_bwd(b, noise)               its argument record's fill and its backward kernel for b.mi.n

// prep, density backward, reduce (+ Adam when adam.p) for one batch; the arguments have been checked and U::once has run
template <class U>
int grad_launch(const qhea_model_desc* desc, const ModelInfo& mi, int64_t batch, int64_t bmax, const double* branch,
                const double* trunk, const double* y, const double* params, const double* ham_diag,
                const typename U::Noise* noise, double inv_bt, double* grad, double* pred, char* ws, hipStream_t st,
                const AdamArgs& adam) {
    const DensGradLayout L = dens_grad_layout(mi, batch);
    double4* gates = reinterpret_cast<double4*>(ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(ws + L.off_cs);
    int rc = launch_prep_model(desc, mi, batch, branch, trunk, params, gates, cs, ws, st);
    if (rc != QHEA_OK) return rc;
    const GradBatch b{desc, mi, params, ham_diag, batch, bmax, gates, cs, pred, reinterpret_cast<double*>(ws + L.off_pred),
                      reinterpret_cast<double*>(ws + L.off_rec), ws, st};
    rc = U::launch_bwd(b, noise);
    if (rc != QHEA_OK) return rc;
    return launch_density_reduce(desc, mi, batch, branch, trunk, y, b.rec, b.pred_ws, inv_bt, grad, adam, st);
}

template <class U>
size_t grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (batch < 0 || model_info(desc, mi) != QHEA_OK) return 0;
    return U::workspace_bytes(mi, batch);
}

template <class U>
int grad_loss_grad(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk, const double* y,
                   const double* params, const double* ham_diag, const typename U::Noise* noise, double inv_batch_total,
                   double* grad, double* pred, void* workspace, size_t workspace_bytes, void* stream) {
    NoisyCall c;
    int rc = U::check(desc, ham_diag, noise, batch, trunk, {branch, y, params, grad}, workspace, stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    if (!U::batch_ok(c.mi, batch)) return QHEA_EINVAL;
    if (!workspace || workspace_bytes < U::workspace_bytes(c.mi, batch)) return QHEA_EWORKSPACE;
    rc = U::once(c.mi, noise, c.ws, batch, c.st);
    if (rc != QHEA_OK) return rc;
    return grad_launch<U>(desc, c.mi, batch, batch, branch, trunk, y, params, ham_diag, noise, inv_batch_total, grad, pred, c.ws,
                          c.st, AdamArgs{});
}

template <class U>
int grad_train_steps(const qhea_model_desc* desc, const TrainCall& call, const double* ham_diag, const typename U::Noise* noise,
                     double lr) {
    if (U::kStepCheckFirst && (!desc || call.n_steps < 0 || call.first_step < 1)) return QHEA_EINVAL;
    NoisyCall c;
    int rc = U::check(desc, ham_diag, noise, call.n_steps, call.trunk,
                      {call.row_begin, call.inv_batch_total, call.branch, call.y, call.grad, call.params, call.exp_avg,
                       call.exp_avg_sq}, call.workspace, call.stream, c);
    if (rc != QHEA_OK) return rc;
    if (call.first_step < 1) return QHEA_EINVAL;
    if (c.empty) return QHEA_OK;
    const int64_t bmax = call_max_batch(call, c.mi.P, *desc);
    if (bmax < 0 || !U::batch_ok(c.mi, bmax)) return QHEA_EINVAL;
    if (!call.workspace || call.workspace_bytes < U::workspace_bytes(c.mi, bmax)) return QHEA_EWORKSPACE;    // (every region grows with the batch)
    rc = U::once(c.mi, noise, c.ws, bmax, c.st);
    if (rc != QHEA_OK) return rc;
    for (int64_t i = 0; i < call.n_steps; ++i) {
        const StepView v = step_view(call, i, *desc);
        rc = grad_launch<U>(desc, c.mi, v.nb, bmax, v.branch, v.trunk, v.y, call.params, ham_diag, noise, v.inv_bt, v.grad, nullptr,
                            c.ws, c.st, adam_step(call, i, lr).adam);
        if (rc != QHEA_OK) return rc;
    }
    return QHEA_OK;
}

}  // namespace
}  // namespace qhea
