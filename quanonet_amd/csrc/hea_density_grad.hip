// hea_density_grad.hip -- qhea_model_loss_grad_noisy_exact / qhea_model_train_steps_noisy_exact: the MSE loss of the exact noisy
// forward (hea_density.hip) and its exact gradient, by the adjoint walk through the density matrix.  The contract is stated in
// include/quanonet_hea.h; tests/density_grad_reference.py restates the walk in numpy.
//
// density_bwd_kernel<N>: one launch per call.  A row's rho and its observable O both live in LDS in the layout of the forward
// (hea_density.hpp; 2 x 16 * 4^n bytes per row; a workgroup is one wave and its 64 / 4^(n-2) rows, at n = 6 the row's four
// waves).  The forward sweep carries rho to the end of the circuit and gives pred; O starts as diag h' (pulled back through the H / H S^dagger of an X / Y read-out); then the
// passes run in reverse.  A reverse pass loads a thread's 16 elements of rho and of O, undoes the two-qubit channel and the CNOT
// (rho: the channel's inverse; O: the channel itself, which is self-adjoint; the CNOT renaming is an involution on both), and
// for each wire whose gates the forward applied in that pass: the one-qubit channel (inverse on rho), then for RY(w2), RZ(w1),
// RY(w0) in turn the trace Im Tr(O sigma rho) followed by the un-rotation of both, and in a block's first sub-layer the
// encoding's channel, trace and RX^dagger.  rho and O are Hermitian, so Tr(O sigma rho) = sum_k conj(O_k) (sigma rho)_k over the
// elements a thread holds: no transposed partner is read.
//
// Sums: a trace is added over a thread's 16 elements, then over the row's lanes by a fixed butterfly, then (n = 6: four waves
// per row) over the waves' partials in wave order through LDS.  The row's d pred / d angle goes to rec[angle][row] in the
// workspace; reduce_density_kernel adds the rows of one parameter in a fixed order (lane l takes rows l, l + 64, ...; the 64
// lane sums by the same butterfly), applies the frequency chain rule and -- train_steps -- the Adam update of hea_adam.hpp.
// No atomics; nothing depends on the grid, and a row's record and pred do not depend on the batch or on other rows.
// What the walk shares with hea_density_device_grad.hip (the same walk over the channel sites of a device noise model) is in
// hea_density_grad.hpp, the body of both units' entry points included (this unit's record is DensGradUnit below);
// launch_density_reduce at the end of this file serves both units.
#include "hea_density_grad.hpp"

namespace qhea {
namespace {

constexpr int kRedWaves = 4;                                             // reduce kernel: one parameter per wave
// the reverse of ring_passes: passes J = N - 1 .. 0 of sub-layer s
template <int N, int J>
__device__ __forceinline__ void ring_passes_back(RowCtx<N>& cx, const DensGradArgs& a, const double2* csr, int s, int col,
                                                 bool enc) {
    if constexpr (J >= 0) {
        using P = Pass<N, J>;
        const int i0 = P::base(cx.rank | opaque_zero()), b = i0 ^ fold(i0) ^ cx.sf;
        double2 e[16], o[16];
        P::load(e, cx.rho, b);
        P::load(o, cx.obs, b);
        undo_cnot2(e, a.r2_keep, a.r2_mix);
        undo_cnot2(o, a.o2_keep, a.o2_mix);
        double tr[kTracesPerPass];
        int idx[kTracesPerPass];
#pragma unroll
        for (int i = 0; i < kTracesPerPass; ++i) { tr[i] = 0.0; idx[i] = -1; }
        const int ans = a.f.E + s * 3 * N;
        if (J <= N - 2) {
            undo_wire<N, 4>(e, o, a, csr, s, col, enc, P::c, tr);
            idx[0] = ans + P::c; idx[1] = ans + N + P::c; idx[2] = ans + 2 * N + P::c; idx[3] = enc ? col + P::c : -1;
        }
        if (J == 0) {
            undo_wire<N, 1>(e, o, a, csr, s, col, enc, P::t, tr + 4);
            idx[4] = ans + P::t; idx[5] = ans + N + P::t; idx[6] = ans + 2 * N + P::t; idx[7] = enc ? col + P::t : -1;
        }
        P::store(e, cx.rho, b);
        P::store(o, cx.obs, b);
        if (J <= N - 2) flush_traces<N>(cx, a, tr, idx);
        else __syncthreads();
        ring_passes_back<N, J - 1>(cx, a, csr, s, col, enc);
    }
}

// the reverse of wire_passes<N, J, 0>: a block without sub-layers, its encoding gates only
template <int N, int J>
__device__ __forceinline__ void encoding_passes_back(RowCtx<N>& cx, const DensGradArgs& a, const double2* csr, int col) {
    if constexpr (J < N) {
        using P = Pass<N, J>;
        const int i0 = P::base(cx.rank | opaque_zero()), b = i0 ^ fold(i0) ^ cx.sf;
        double2 e[16], o[16];
        P::load(e, cx.rho, b);
        P::load(o, cx.obs, b);
        double tr[kTracesPerPass];
        int idx[kTracesPerPass];
#pragma unroll
        for (int i = 0; i < kTracesPerPass; ++i) { tr[i] = 0.0; idx[i] = -1; }
        undo_encoding<1>(e, o, a, csr[col + P::t], tr);
        idx[3] = col + P::t;
        if (J + 1 < N) {
            undo_encoding<4>(e, o, a, csr[col + P::c], tr + 4);
            idx[7] = col + P::c;
        }
        P::store(e, cx.rho, b);
        P::store(o, cx.obs, b);
        flush_traces<N>(cx, a, tr, idx);
        encoding_passes_back<N, J + 2>(cx, a, csr, col);
    }
}

template <int N>
__global__ __launch_bounds__(bwd_threads<N>()) void density_bwd_kernel(DensGradArgs a) {
    using C = RowCtx<N>;
    constexpr int TPR = C::TPR, RPW = bwd_threads<N>() / TPR, D = 1 << N, NE = 1 << (2 * N);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];      // rho, O, h'[D], the waves' trace partials
    double2* state = reinterpret_cast<double2*>(dens_lds);
    double* hv = reinterpret_cast<double*>(dens_lds + 2 * RPW * NE * sizeof(double2));
    const int tid = threadIdx.x, slot = tid / TPR, rank = tid % TPR;
    long r = (long)blockIdx.x * RPW + slot;
    const bool live = r < a.f.B;
    if (!live) r = a.f.B - 1;                                            // a tail slot repeats the last row and stores nothing
    const double2* csr = a.f.cs + r * a.f.E;
    C cx;
    cx.rho = state + slot * NE;
    cx.obs = state + RPW * NE + slot * NE;
    cx.red = hv + D;
    cx.rank = rank; cx.sf = slot_fold<N>(slot); cx.parity = 0;
    cx.r = r; cx.B = a.f.B; cx.live = live;
    double2* row = cx.rho;
    const int sf = cx.sf;

    // value table under the readout confusion: n two-point mixes of h
    double h = 0.0;
    if (tid < D) h = a.f.diag ? a.f.diag[tid] : a.f.off + a.f.co * (double)(N - 2 * (int)__popc(tid));
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (tid < D) hv[tid] = h;
        __syncthreads();
        if (tid < D) h = (1.0 - a.f.q) * h + a.f.q * hv[tid ^ (1 << i)];
        __syncthreads();
    }
    if (tid < D) hv[tid] = h;

    // forward sweep: the passes of density_fwd_kernel
    int s = 0, col = 0;
    bool first = true;
    for (int g = 0; g < 2; ++g) {
        for (int b = 0; b < a.f.nb[g]; ++b) {
            if (a.f.ld[g] == 0) {
                wire_passes<N, 0, 0>(row, rank, sf, a.f, csr, col, first);
                first = false;
            }
            for (int l = 0; l < a.f.ld[g]; ++l, ++s) {
                ring_passes<N, 0>(row, rank, sf, a.f, csr, s, col, l == 0, first);
                first = false;
            }
            col += N;
        }
    }
    if (first) {                                                         // no block at all: rho = |0><0|
        for (int i = rank; i < NE; i += TPR) row[i] = make_double2(0.0, 0.0);
        __syncthreads();
        if (rank == 0) row[fold(0) ^ sf] = make_double2(1.0, 0.0);
        __syncthreads();
    }
    if (a.f.pauli == QHEA_PAULI_X) wire_passes<N, 0, 1>(row, rank, sf, a.f, csr, 0, false);
    else if (a.f.pauli == QHEA_PAULI_Y) wire_passes<N, 0, 2>(row, rank, sf, a.f, csr, 0, false);

    if (rank == 0 && live) {
        double m1 = 0.0;
        for (int k = 0; k < D; ++k) {
            int i = 0;
#pragma unroll
            for (int w = 0; w < N; ++w) i |= ((k >> w) & 1) * (3 << (2 * w));
            m1 += row[i ^ fold(i) ^ sf].x * hv[k];
        }
        const double p = m1 + (a.f.bias ? a.f.bias[0] : 0.0);
        a.pred_ws[r] = p;
        if (a.f.pred) a.f.pred[r] = p;
    }

    // O = diag (h' - mean h') in the read-out basis.  The identity component of O is a fixed point of the pull-back (every
    // channel here is unital and self-adjoint) and Im Tr(sigma rho) = 0, so it carries no gradient; left in, it meets the
    // rounding residue of the inverse walk on rho, which grows with A while the rest of O shrinks with 1 / A: a read-out
    // offset of 0.5 cost 8e-7 on gradients of 6e-11 at log10 A = 11.99.  pred keeps the whole h'.
    double hbar = 0.0;
    for (int k = 0; k < D; ++k) hbar += hv[k];
    hbar *= 1.0 / D;
    for (int i = rank; i < NE; i += TPR) {
        int k = 0;
        bool diag = true;
#pragma unroll
        for (int w = 0; w < N; ++w) {
            const int rb = (i >> (2 * w)) & 1, cb = (i >> (2 * w + 1)) & 1;
            diag = diag && rb == cb;
            k |= rb << w;
        }
        cx.obs[i ^ fold(i) ^ sf] = make_double2(diag ? hv[k] - hbar : 0.0, 0.0);
    }
    __syncthreads();
    // back to the computational basis: rho and O through the daggers of the basis change
    if (a.f.pauli == QHEA_PAULI_X) {
        basis_passes_back<N, 0, 3>(cx.rho, rank, sf);
        basis_passes_back<N, 0, 3>(cx.obs, rank, sf);
    } else if (a.f.pauli == QHEA_PAULI_Y) {
        basis_passes_back<N, 0, 4>(cx.rho, rank, sf);
        basis_passes_back<N, 0, 4>(cx.obs, rank, sf);
    }

    // reverse walk: blocks, sub-layers and passes in reverse order
    for (int g = 1; g >= 0; --g) {
        for (int b = a.f.nb[g] - 1; b >= 0; --b) {
            col -= N;
            for (int l = a.f.ld[g] - 1; l >= 0; --l) {
                --s;
                ring_passes_back<N, N - 1>(cx, a, csr, s, col, l == 0);
            }
            if (a.f.ld[g] == 0) encoding_passes_back<N, 0>(cx, a, csr, col);
        }
    }
}

// Where output o of the reduce kernel comes from
struct DensRed {
    const double* rec; const double* pred; const double* y;
    const double* in[2];                    // the segments' inputs
    long B, P, off_ans, off_bias;
    long off_w[2], off_b[2];
    int ncols[2], width[2];
    int E, nans;
    double inv_bt;
    double* grad;                           // [P + 2]
    AdamArgs adam;
};

// One wave per output: the P gradients, then sum (pred - y)^2 and sum y^2.  Lane l adds rows l, l + 64, ... in order, the lanes'
// sums meet in a fixed butterfly; lane 0 writes the result and, with adam.p, applies the update of its parameter.
__global__ __launch_bounds__(64 * kRedWaves) void reduce_density_kernel(DensRed a) {
    const long o = (long)blockIdx.x * kRedWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (o >= a.P + 2) return;                                            // whole waves
    // kind: 0 weighted record column, 1 the same times the tiled input, 2 sum g, 3 sse, 4 sum y^2
    int kind = -1, colx = 0, seg = 0, e = 0;
    if (o == a.P) kind = 3;
    else if (o == a.P + 1) kind = 4;
    else if (o == a.off_bias) kind = 2;
    else if (o >= a.off_ans && o < a.off_ans + a.nans) { kind = 0; colx = a.E + (int)(o - a.off_ans); }
    else {
        for (int sg = 0; sg < 2; ++sg) {
            if (a.off_w[sg] >= 0 && o >= a.off_w[sg] && o < a.off_w[sg] + a.ncols[sg]) { kind = 1; seg = sg; e = (int)(o - a.off_w[sg]); }
            if (a.off_b[sg] >= 0 && o >= a.off_b[sg] && o < a.off_b[sg] + a.ncols[sg]) { kind = 0; seg = sg; e = (int)(o - a.off_b[sg]); }
        }
        colx = (seg ? a.ncols[0] : 0) + e;
    }
    double acc = 0.0;
    if (kind >= 0) {
        for (long b = lane; b < a.B; b += 64) {
            const double yb = a.y[b], d = a.pred[b] - yb;
            const double g = 2.0 * d * a.inv_bt;
            double t;
            if (kind == 0) t = g * a.rec[(long)colx * a.B + b];
            else if (kind == 1) t = g * a.rec[(long)colx * a.B + b] * a.in[seg][b * a.width[seg] + e % a.width[seg]];
            else if (kind == 2) t = g;
            else if (kind == 3) t = d * d;
            else t = yb * yb;
            acc += t;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) {
        a.grad[o] = acc;
        if (a.adam.p && o < a.P) adam_update(a.adam, o, acc);
    }
}

// The unit record of grad_loss_grad / grad_train_steps (hea_density_grad.hpp): the uniform channels of a qhea_noise
struct DensGradUnit {
    using Noise = qhea_noise;
    static constexpr bool kStepCheckFirst = true;
    static size_t workspace_bytes(const ModelInfo& mi, int64_t B) { return dens_grad_layout(mi, B).total; }
    static int check(const qhea_model_desc* desc, const double* ham_diag, const qhea_noise* noise, int64_t count,
                     const double* trunk, std::initializer_list<const void*> required, void* workspace, void* stream,
                     NoisyCall& c) {
        return noisy_call_check({QHEA_MIN_QUBITS, 6 /* 2 x 4^n elements per row in LDS */, false, true}, desc, ham_diag, noise, 0,
                                count, trunk, required, workspace, stream, c);
    }
    static bool batch_ok(const ModelInfo&, int64_t) { return true; }
    static int once(const ModelInfo&, const qhea_noise*, char*, int64_t, hipStream_t) { return QHEA_OK; }
    static int launch_bwd(const GradBatch& b, const qhea_noise* noise) {
        const DensGradArgs a = dens_grad_args(b, noise);
        return dispatch_n(b.mi.n, [&](auto n) { return launch_density_bwd<n()>(density_bwd_kernel<n()>, a.f.B, a, b.st); });
    }
};

}  // namespace

int launch_density_reduce(const qhea_model_desc* desc, const ModelInfo& mi, int64_t batch, const double* branch,
                          const double* trunk, const double* y, const double* rec, const double* pred, double inv_bt,
                          double* grad, const AdamArgs& adam, hipStream_t st) {
    DensRed d{};
    d.rec = rec; d.pred = pred; d.y = y;
    d.in[0] = desc->model == QHEA_MODEL_QUANONET ? trunk : branch; d.in[1] = branch;
    d.B = batch; d.P = mi.P; d.off_ans = mi.off_ans; d.off_bias = mi.off_bias;
    for (int s = 0; s < 2; ++s) {
        d.off_w[s] = mi.off_w[s]; d.off_b[s] = mi.off_b[s]; d.ncols[s] = (int)mi.enc_cols[s]; d.width[s] = mi.width[s];
    }
    d.E = (int)mi.sh.E; d.nans = 3 * mi.n * (int)mi.sh.blk;
    d.inv_bt = inv_bt; d.grad = grad; d.adam = adam;
    hipLaunchKernelGGL(reduce_density_kernel, dim3((unsigned)((mi.P + 2 + kRedWaves - 1) / kRedWaves)), dim3(64 * kRedWaves), 0,
                       st, d);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_exact_noisy_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    return grad_workspace_bytes<DensGradUnit>(desc, batch);
}

double qhea_model_exact_noisy_log10_amplification(const qhea_model_desc* desc, const qhea_noise* noise) {
    ModelInfo mi;
    if (model_info(desc, mi) != QHEA_OK || !rates_ok(noise)) return NAN;
    return log10_amplification(mi, noise);
}

int qhea_model_loss_grad_noisy_exact(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                                     const double* y, const double* params, const double* ham_diag, const qhea_noise* noise,
                                     double inv_batch_total, double* grad, double* pred, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return grad_loss_grad<DensGradUnit>(desc, batch, branch, trunk, y, params, ham_diag, noise, inv_batch_total, grad, pred,
                                        workspace, workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_exact(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                       const double* branch, const double* trunk, const double* y, double* params,
                                       const double* ham_diag, const qhea_noise* noise, const double* inv_batch_total,
                                       double* grad, int64_t grad_stride, double* exp_avg, double* exp_avg_sq,
                                       int64_t first_step, double lr, double beta1, double beta2, double eps,
                                       double weight_decay, void* workspace, size_t workspace_bytes, void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return grad_train_steps<DensGradUnit>(desc, call, ham_diag, noise, lr);
}

}  // extern "C"
