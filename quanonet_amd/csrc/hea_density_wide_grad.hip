// hea_density_wide_grad.hip -- qhea_model_loss_grad_noisy_exact_wide / qhea_model_train_steps_noisy_exact_wide: the MSE loss of
// the exact noisy forward and its exact gradient (the quantity and the adjoint walk of hea_density_grad.hip) for n = 7, 8, 9,
// on the tiles of hea_density_wide.hip.  rho and the observable O of all rows of the call live in the workspace, 4^n x 16 bytes
// per row each, in hea_density.hip's index layout; row r of rho is at rho + r 4^n, row r of O at obs + r 4^n.
//
// Forward sweep: the value-table kernel, the stage launches and the read-out kernel of hea_density_wide_stages.hpp, word for
// word, so a row's pred is what qhea_model_forward_noisy_exact_wide returns for it.
// O_N: one launch writes O = diag(h' - mean h'), zero elsewhere (the mean is taken out for the reason given in
// density_bwd_kernel).  For an X / Y read-out rho and O then go through the daggers of the basis change as one-qubit stages:
// stage B serves wires 6..n-1, stage A wires 0..5.
// Reverse stages: a reverse sub-layer is stage B with the ring passes j = n-1..5, then stage A with j = 4..0, each one launch
// over rows x 4^(n-6) workgroups of 256 threads.  A workgroup loads its tile of rho and its tile of O (2 x 64 KiB of LDS, the
// residency of density_bwd_kernel<6>: one workgroup per CU), runs the body of ring_passes_back on the local pass
// Pass<6, j < 5 ? j : j - n + 6> -- undo_cnot2 on both, then per pending wire undo_wire of hea_density_grad.hpp, with the
// forward's pending-gate rule in global wires and the angle tables indexed by the circuit's n and the global wire -- and stores
// both tiles.  A block without sub-layers is the reverse of wide_wire_pass, stage B then stage A.
//
// Traces across tiles: a trace is a sum over the 4^(n-6) tiles of a row, which sit in different workgroups.  A workgroup adds
// its threads' shares by flush_traces<6> (the butterfly over a wave, the four waves in wave order) and writes one partial per
// (angle, row, tile); every angle belongs to exactly one stage launch, so every partial is written exactly once per step.  The
// partial buffer holds ALL angles of the circuit, (E + 3 n blk) x rows x 4^(n-6) doubles -- 7 to 12 % of the two matrices for
// the 60-sub-layer models of DESIGN.md 7v -- and ONE fold launch at the end adds the tiles in tile order 0, 1, .. into
// rec[angle][row] (a fold per stage would need 24 angles' room only, but two more launches per sub-layer).  The fold launch also
// copies pred to the caller.  reduce_density_kernel then adds the rows as in every density-matrix unit.  No atomics, no flags:
// the launch boundary is the only synchronisation between workgroups, and a row's pred and records are bitwise independent of
// the batch, the grid and the chunking.
// What the device-noise unit hea_density_device_wide_grad.hip shares with this one -- tile_ctx, the reverse one-qubit stages, the
// O_N and fold kernels, the layout -- sits in hea_density_wide_grad.hpp.  (The stages header comes first: the two kernels that
// are no templates, its value-table kernel and the fold kernel, then stand in the object in the order they always had.)
#include "hea_density_wide_stages.hpp"
#include "hea_density_wide_grad.hpp"

namespace qhea {
namespace {

// ring pass J of the circuit's n wires in reverse, on the tile that holds both of its wires: the body of ring_passes_back
template <int N, int J>
__device__ __forceinline__ void wide_ring_pass_back(RowCtx<6>& cx, const DensGradArgs& a, const double2* csr, int s, int col,
                                                    bool enc) {
    using P = Pass<6, (J < 5 ? J : J - N + 6)>;
    const int i0 = P::base(cx.rank | opaque_zero()), b = i0 ^ fold(i0);
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
        constexpr int q = J + 1;
        undo_wire<N, 4>(e, o, a, csr, s, col, enc, q, tr);
        idx[0] = ans + q; idx[1] = ans + N + q; idx[2] = ans + 2 * N + q; idx[3] = enc ? col + q : -1;
    }
    if (J == 0) {
        undo_wire<N, 1>(e, o, a, csr, s, col, enc, 0, tr + 4);
        idx[4] = ans; idx[5] = ans + N; idx[6] = ans + 2 * N; idx[7] = enc ? col : -1;
    }
    P::store(e, cx.rho, b);
    P::store(o, cx.obs, b);
    if (J <= N - 2) flush_traces<6>(cx, a, tr, idx);
    else __syncthreads();
}
template <int N, int J, int JEND>                                        // passes J, J - 1, .., JEND
__device__ __forceinline__ void wide_ring_passes_back(RowCtx<6>& cx, const DensGradArgs& a, const double2* csr, int s, int col,
                                                      bool enc) {
    if constexpr (J >= JEND) {
        wide_ring_pass_back<N, J>(cx, a, csr, s, col, enc);
        wide_ring_passes_back<N, J - 1, JEND>(cx, a, csr, s, col, enc);
    }
}

// a reverse ring stage of sub-layer s: stage B passes n-1..5, stage A passes 4..0.  a.rec: the partials.  Grid: rows x 4^(n-6)
// workgroups, tile fastest
template <int N, int STAGE>
__global__ __launch_bounds__(kDensThreads) void density_wide_ring_back_kernel(DensGradArgs a, double2* rho, double2* obs, int s,
                                                                              int col, int enc) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    double2* rrow = rho + ((size_t)r << (2 * N));
    double2* orow = obs + ((size_t)r << (2 * N));
    const double2* csr = a.f.cs + r * a.f.E;
    RowCtx<6> cx = tile_ctx<N>(lds, tid, r, tile, a.f.B);
    tile_load<N, STAGE>(cx.rho, rrow, tile, tid, false);
    tile_load<N, STAGE>(cx.obs, orow, tile, tid, false);
    if (STAGE == 0) wide_ring_passes_back<N, 4, 0>(cx, a, csr, s, col, enc != 0);
    else wide_ring_passes_back<N, N - 1, 5>(cx, a, csr, s, col, enc != 0);
    tile_store<N, STAGE>(cx.rho, rrow, tile, tid);
    tile_store<N, STAGE>(cx.obs, orow, tile, tid);
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// every launch of one batch between the prep kernel and the reduce kernel, in stream order.  a.rec: the records
template <int N>
int launch_density_wide_grad(DensGradArgs a, double* pred, double* hv, double* partial, double2* rho, double2* obs, long nrec,
                             hipStream_t st) {
    constexpr int tiles = 1 << (2 * (N - 6));
    const dim3 grid((unsigned)(a.f.B << (2 * (N - 6)))), block(kDensThreads);
    double* rec = a.rec;
    a.rec = partial;                                                     // what the stages' flush_traces writes
    a.f.pred = a.pred_ws; a.f.sd = nullptr;                              // the read-out kernel's pred
    hipLaunchKernelGGL(density_wide_values_kernel, dim3(1), dim3(512), 0, st, a.f, N, hv);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    int rc = launch_density_wide<N>(a.f, rho, hv, st);
    if (rc != QHEA_OK) return rc;
    hipLaunchKernelGGL(density_wide_observable_kernel<N>, grid, block, 0, st, hv, obs);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    if (a.f.pauli != QHEA_PAULI_Z) {
        const int kind = a.f.pauli == QHEA_PAULI_X ? 3 : 4;
        rc = launch_dynamic_lds(density_wide_wires_back_kernel<N, 1, true>, grid, block, kWideBwdLds, st, a, rho, obs, 0, kind);
        if (rc == QHEA_OK)
            rc = launch_dynamic_lds(density_wide_wires_back_kernel<N, 0, true>, grid, block, kWideBwdLds, st, a, rho, obs, 0, kind);
        if (rc != QHEA_OK) return rc;
    }
    int s = a.f.nb[0] * a.f.ld[0] + a.f.nb[1] * a.f.ld[1], col = N * (a.f.nb[0] + a.f.nb[1]);
    for (int g = 1; g >= 0; --g) {
        for (int b = a.f.nb[g] - 1; b >= 0; --b) {
            col -= N;
            for (int l = a.f.ld[g] - 1; l >= 0; --l) {
                --s;
                rc = launch_dynamic_lds(density_wide_ring_back_kernel<N, 1>, grid, block, kWideBwdLds, st, a, rho, obs, s, col,
                                        (int)(l == 0));
                if (rc == QHEA_OK)
                    rc = launch_dynamic_lds(density_wide_ring_back_kernel<N, 0>, grid, block, kWideBwdLds, st, a, rho, obs, s, col,
                                            (int)(l == 0));
                if (rc != QHEA_OK) return rc;
            }
            if (a.f.ld[g] == 0) {
                rc = launch_dynamic_lds(density_wide_wires_back_kernel<N, 1, false>, grid, block, kWideBwdLds, st, a, rho, obs, col, 0);
                if (rc == QHEA_OK)
                    rc = launch_dynamic_lds(density_wide_wires_back_kernel<N, 0, false>, grid, block, kWideBwdLds, st, a, rho, obs, col,
                                            0);
                if (rc != QHEA_OK) return rc;
            }
        }
    }
    const long nsum = nrec * a.f.B, nthr = nsum > a.f.B ? nsum : a.f.B;
    hipLaunchKernelGGL(density_wide_fold_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, partial, rec, nsum, tiles,
                       a.pred_ws, pred, a.f.B);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

// The unit record of grad_loss_grad / grad_train_steps (hea_density_grad.hpp): the uniform channels of a qhea_noise on tiles.
// The many-launch sequence fits the shared body as it is: that body hands launch_bwd one batch between its prep and its reduce
// launch, and this unit's regions follow dens_grad_layout's in the workspace.
struct WideGradUnit {
    using Noise = qhea_noise;
    static constexpr bool kStepCheckFirst = true;
    static size_t workspace_bytes(const ModelInfo& mi, int64_t B) { return wide_grad_layout(mi, B).total; }
    static int check(const qhea_model_desc* desc, const double* ham_diag, const qhea_noise* noise, int64_t count,
                     const double* trunk, std::initializer_list<const void*> required, void* workspace, void* stream,
                     NoisyCall& c) {
        return noisy_call_check({7, 9 /* rho and O in the workspace, six wires at a time in LDS */, false, true}, desc, ham_diag,
                                noise, 0, count, trunk, required, workspace, stream, c);
    }
    // a stage has one workgroup per (row, tile)
    static bool batch_ok(const ModelInfo& mi, int64_t B) { return B <= (int64_t)INT_MAX >> (2 * (mi.n - 6)); }
    static int once(const ModelInfo&, const qhea_noise*, char*, int64_t, hipStream_t) { return QHEA_OK; }
    static int launch_bwd(const GradBatch& b, const qhea_noise* noise) {
        DensGradArgs a = dens_grad_args(b, noise);
        const WideGradLayout L = wide_grad_layout(b.mi, b.batch);
        double* hv = reinterpret_cast<double*>(b.ws + L.off_hv);
        double* partial = reinterpret_cast<double*>(b.ws + L.off_partial);
        double2* rho = reinterpret_cast<double2*>(b.ws + L.off_rho);
        double2* obs = reinterpret_cast<double2*>(b.ws + L.off_obs);
        const long nrec = (long)b.mi.sh.E + 3L * b.mi.n * b.mi.sh.blk;
        return dispatch_wide_n(b.mi.n, [&](auto n) {
            return launch_density_wide_grad<n()>(a, b.pred, hv, partial, rho, obs, nrec, b.st);
        });
    }
};

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_exact_noisy_wide_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (batch < 0 || model_info(desc, mi) != QHEA_OK || mi.n < 7 || mi.n > 9) return 0;
    return WideGradUnit::workspace_bytes(mi, batch);
}

int qhea_model_loss_grad_noisy_exact_wide(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                                          const double* y, const double* params, const double* ham_diag, const qhea_noise* noise,
                                          double inv_batch_total, double* grad, double* pred, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    return grad_loss_grad<WideGradUnit>(desc, batch, branch, trunk, y, params, ham_diag, noise, inv_batch_total, grad, pred,
                                        workspace, workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_exact_wide(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                            const double* branch, const double* trunk, const double* y, double* params,
                                            const double* ham_diag, const qhea_noise* noise, const double* inv_batch_total,
                                            double* grad, int64_t grad_stride, double* exp_avg, double* exp_avg_sq,
                                            int64_t first_step, double lr, double beta1, double beta2, double eps,
                                            double weight_decay, void* workspace, size_t workspace_bytes, void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return grad_train_steps<WideGradUnit>(desc, call, ham_diag, noise, lr);
}

}  // extern "C"
