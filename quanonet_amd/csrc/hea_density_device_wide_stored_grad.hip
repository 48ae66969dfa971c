// hea_density_device_wide_stored_grad.hip -- qhea_model_loss_grad_noisy_device_exact_wide_stored /
// qhea_model_train_steps_noisy_device_exact_wide_stored: the loss and exact gradient of hea_density_device_wide_grad.hip (n = 7,
// 8, 9 under the calibrated device noise model, on tiles) past that unit's guard, with rho replayed from stored states as
// hea_density_device_grad.hip's stored-state kernel does for n <= 6.
//
// A unit is one sub-layer (a block's first sub-layer carries the block's encoding) or the encoding of a block without
// sub-layers; U = sub-layers + blocks without sub-layers.  snap[u] holds every row's rho after unit u, row r at element
// (u B + r) 4^n (size_t arithmetic), behind the regions of the inverse unit's workspace.
//
// Forward sweep: launch_density_dev_wide's sequence with the same value-table, stage B and read-out kernels; stage A of unit u
// is the source/destination form below (density_dev_wide_ring_to_kernel, density_dev_wide_wires_to_kernel: the stage A kernels
// of hea_density_device_wide_stages.hpp, statement for statement, loading the row from one base and storing it to another): it
// loads snap[u-1] (u = 0: nothing, the `first` rule) and stores snap[u]; stage B of unit u works in place on snap[u].  Stage A of
// an X / Y read-out basis change loads snap[U-1] and stores to the running rho buffer (the inverse unit's rho region), stage B
// works there, and the read-out kernel reads the running buffer; a Z read-out reads snap[U-1].  The arithmetic is untouched.
//
// Reverse walk: the passes of hea_density_device_wide_grad.hpp (dev_wide_ring_passes_back, dev_wide_wire_pass_back: the same
// table, undo_site, undo_cnot2, undo_rotations, dev_undo_encoding, trace partials), O_N, the dagger-of-basis stages, fold and
// reduce as in the inverse unit.  Only where rho comes from and goes differs: a unit's first reverse stage (stage B) loads its rho
// tile from snap[u] and stores it to the running buffer -- the snapshots are read-only after the forward sweep, and no stage
// reads and writes the same rho row through two names --, its second stage (stage A) loads what stage B stored and stores no
// rho at all: the next unit starts from snap[u-1].  So between two stored states rho walks back through one unit only, and
// the guard is asked of the largest single unit (DevStoredGradUnit's rule).  O is walked in place as before.
// A circuit without blocks has U = 0, takes no snapshot and runs the inverse unit's launches.
//
// The pointers are kernel arguments, wave-uniform, and live in scalar registers: the forms cost no vector register (profiles/
// r42_resource_usage.txt: no scratch, no spill).  By byte count a reverse unit moves one rho store less than the inverse unit's
// (11 of a sub-layer's 12 row transfers): an estimate; DESIGN.md 7x has what was measured.
//
// No atomics, no flags, no spinning, no grid barrier: the launch boundary is the only synchronisation between workgroups, and
// a row's pred and records are bitwise independent of the batch, the grid and the chunking.
#include "hea_density_device_wide_grad.hpp"

namespace qhea {
namespace {

// ---- forward stage A, from one row base to another ----

// density_dev_wide_ring_kernel<N, 0>: passes 0..4 of sub-layer s
template <int N>
__global__ __launch_bounds__(kDensThreads) void density_dev_wide_ring_to_kernel(DevStageArgs a, const double2* src, double2* dst,
                                                                                int s, int col, int enc, int first) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    const size_t row = (size_t)r << (2 * N);
    const double2* csr = a.cs + r * a.E;
    tile_load<N, 0>(lds, src + row, tile, tid, first != 0);
    dev_wide_ring_passes<N, 0, 5>(lds, tid, a, csr, s, col, enc != 0);
    tile_store<N, 0>(lds, dst + row, tile, tid);
}

// density_dev_wide_wires_kernel<N, 0>: wires 0..5; kind 0 = a block's encoding, 1 / 2 = the read-out basis change
template <int N>
__global__ __launch_bounds__(kDensThreads) void density_dev_wide_wires_to_kernel(DevStageArgs a, const double2* src, double2* dst,
                                                                                 int col, int kind, int first) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    const size_t row = (size_t)r << (2 * N);
    const double2* csr = a.cs + r * a.E;
    tile_load<N, 0>(lds, src + row, tile, tid, first != 0);
    dev_wide_wire_pass<N, 0, 0>(lds, tid, a, csr, col, kind);
    dev_wide_wire_pass<N, 0, 2>(lds, tid, a, csr, col, kind);
    dev_wide_wire_pass<N, 0, 4>(lds, tid, a, csr, col, kind);
    tile_store<N, 0>(lds, dst + row, tile, tid);
}

// ---- reverse stages: rho from `src`; stage B stores it to `rho`, stage A stores none ----

// density_dev_wide_ring_back_kernel<N, STAGE>
template <int N, int STAGE>
__global__ __launch_bounds__(kDensThreads) void density_dev_wide_ring_back_from_kernel(DevWideGradArgs a, const double2* src,
                                                                                       double2* rho, double2* obs, int s, int col,
                                                                                       int enc) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    const size_t row = (size_t)r << (2 * N);
    double2* orow = obs + row;
    const double2* csr = a.cs + r * a.E;
    RowCtx<6> cx = tile_ctx<N>(lds, tid, r, tile, a.B);
    tile_load<N, STAGE>(cx.rho, src + row, tile, tid, false);
    tile_load<N, STAGE>(cx.obs, orow, tile, tid, false);
    if (STAGE == 0) dev_wide_ring_passes_back<N, 4, 0>(cx, a, csr, s, col, enc != 0);
    else dev_wide_ring_passes_back<N, N - 1, 5>(cx, a, csr, s, col, enc != 0);
    if (STAGE == 1) tile_store<N, STAGE>(cx.rho, rho + row, tile, tid);
    tile_store<N, STAGE>(cx.obs, orow, tile, tid);
}

// density_dev_wide_enc_back_kernel<N, STAGE>
template <int N, int STAGE>
__global__ __launch_bounds__(kDensThreads) void density_dev_wide_enc_back_from_kernel(DevWideGradArgs a, const double2* src,
                                                                                      double2* rho, double2* obs, int col) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    const size_t row = (size_t)r << (2 * N);
    double2* orow = obs + row;
    const double2* csr = a.cs + r * a.E;
    RowCtx<6> cx = tile_ctx<N>(lds, tid, r, tile, a.B);
    tile_load<N, STAGE>(cx.rho, src + row, tile, tid, false);
    tile_load<N, STAGE>(cx.obs, orow, tile, tid, false);
    dev_wide_wire_pass_back<N, STAGE, 4>(cx, a, csr, col);
    dev_wide_wire_pass_back<N, STAGE, 2>(cx, a, csr, col);
    dev_wide_wire_pass_back<N, STAGE, 0>(cx, a, csr, col);
    if (STAGE == 1) tile_store<N, STAGE>(cx.rho, rho + row, tile, tid);
    tile_store<N, STAGE>(cx.obs, orow, tile, tid);
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// every launch of one batch between the prep kernel and the reduce kernel, in stream order; U >= 1 units, snap[u] at
// snap + u B 4^n
template <int N>
int launch_density_dev_wide_stored_grad(const DevWideGradCall& c, double* hv, double* partial, double2* rho, double2* obs,
                                        double2* snap, long nrec, hipStream_t st) {
    constexpr int tiles = 1 << (2 * (N - 6));
    const long B = c.bwd.B;
    const size_t slot = (size_t)B << (2 * N);                            // elements of one snapshot
    const dim3 grid((unsigned)(B << (2 * (N - 6)))), block(kDensThreads);
    hipLaunchKernelGGL(density_dev_wide_values_kernel<N>, dim3(1), dim3(512), 0, st, c.values, hv);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    // forward sweep: launch_density_dev_wide with stage A of unit u from snap[u - 1] to snap[u]
    const DevWideCall& f = c.fwd;
    int rc = QHEA_OK;
    long u = 0;
    int s = 0, col = 0;
    for (int g = 0; g < 2; ++g) {
        for (int b = 0; b < f.nb[g]; ++b) {
            if (f.ld[g] == 0) {
                double2* cur = snap + (size_t)u * slot;
                rc = launch_dynamic_lds(density_dev_wide_wires_to_kernel<N>, grid, block, kDensStateBytes, st, f.stage[0],
                                        (const double2*)(u ? cur - slot : cur), cur, col, 0, (int)(u == 0));
                if (rc == QHEA_OK)
                    rc = launch_dynamic_lds(density_dev_wide_wires_kernel<N, 1>, grid, block, kDensStateBytes, st, f.stage[1], cur,
                                            col, 0, 0);
                if (rc != QHEA_OK) return rc;
                ++u;
            }
            for (int l = 0; l < f.ld[g]; ++l, ++s, ++u) {
                double2* cur = snap + (size_t)u * slot;
                rc = launch_dynamic_lds(density_dev_wide_ring_to_kernel<N>, grid, block, kDensStateBytes, st, f.stage[0],
                                        (const double2*)(u ? cur - slot : cur), cur, s, col, (int)(l == 0), (int)(u == 0));
                if (rc == QHEA_OK)
                    rc = launch_dynamic_lds(density_dev_wide_ring_kernel<N, 1>, grid, block, kDensStateBytes, st, f.stage[1], cur, s,
                                            col, (int)(l == 0), 0);
                if (rc != QHEA_OK) return rc;
            }
            col += N;
        }
    }
    const double2* last = snap + (size_t)(u - 1) * slot;
    if (f.pauli != QHEA_PAULI_Z) {
        const int kind = f.pauli == QHEA_PAULI_X ? 1 : 2;
        rc = launch_dynamic_lds(density_dev_wide_wires_to_kernel<N>, grid, block, kDensStateBytes, st, f.stage[0], last, rho, 0, kind,
                                0);
        if (rc == QHEA_OK)
            rc = launch_dynamic_lds(density_dev_wide_wires_kernel<N, 1>, grid, block, kDensStateBytes, st, f.stage[1], rho, 0, kind,
                                    0);
        if (rc != QHEA_OK) return rc;
        last = rho;
    }
    hipLaunchKernelGGL(density_wide_readout_kernel<N>, dim3((unsigned)B), dim3(64), 0, st, f.out, last, hv);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    hipLaunchKernelGGL(density_wide_observable_kernel<N>, grid, block, 0, st, hv, obs);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    if (f.pauli != QHEA_PAULI_Z) {                                       // O through the daggers; rho with it, read by nobody
        const int kind = f.pauli == QHEA_PAULI_X ? 3 : 4;
        rc = launch_dynamic_lds(density_wide_wires_back_kernel<N, 1, true>, grid, block, kWideBwdLds, st, c.basis, rho, obs, 0, kind);
        if (rc == QHEA_OK)
            rc = launch_dynamic_lds(density_wide_wires_back_kernel<N, 0, true>, grid, block, kWideBwdLds, st, c.basis, rho, obs, 0,
                                    kind);
        if (rc != QHEA_OK) return rc;
    }
    // reverse walk: unit u from snap[u]
    const DevWideGradArgs& a = c.bwd;
    for (int g = 1; g >= 0; --g) {
        for (int b = f.nb[g] - 1; b >= 0; --b) {
            col -= N;
            for (int l = f.ld[g] - 1; l >= 0; --l) {
                --s; --u;
                rc = launch_dynamic_lds(density_dev_wide_ring_back_from_kernel<N, 1>, grid, block, kWideBwdLds, st, a,
                                        (const double2*)(snap + (size_t)u * slot), rho, obs, s, col, (int)(l == 0));
                if (rc == QHEA_OK)
                    rc = launch_dynamic_lds(density_dev_wide_ring_back_from_kernel<N, 0>, grid, block, kWideBwdLds, st, a,
                                            (const double2*)rho, rho, obs, s, col, (int)(l == 0));
                if (rc != QHEA_OK) return rc;
            }
            if (f.ld[g] == 0) {
                --u;
                rc = launch_dynamic_lds(density_dev_wide_enc_back_from_kernel<N, 1>, grid, block, kWideBwdLds, st, a,
                                        (const double2*)(snap + (size_t)u * slot), rho, obs, col);
                if (rc == QHEA_OK)
                    rc = launch_dynamic_lds(density_dev_wide_enc_back_from_kernel<N, 0>, grid, block, kWideBwdLds, st, a,
                                            (const double2*)rho, rho, obs, col);
                if (rc != QHEA_OK) return rc;
            }
        }
    }
    const long nsum = nrec * B, nthr = nsum > B ? nsum : B;
    hipLaunchKernelGGL(density_wide_fold_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, partial, c.rec, nsum, tiles,
                       f.out.pred, c.pred, B);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

// The unit record of the stored-state calls on tiles: DevWideGradUnit with the snapshot region behind its workspace and the
// guard asked of the largest single unit, as DevStoredGradUnit of hea_density_device_grad.hip.  Table, checks, prep and reduce
// launches are the inverse unit's.
struct DevWideStoredGradUnit : DevWideGradUnit {
    // U: sub-layers, plus the blocks without any (one encoding-only unit each)
    static size_t units(const ModelInfo& mi) {
        size_t u = 0;
        for (int g = 0; g < 2; ++g) u += (size_t)mi.nb[g] * (size_t)(mi.ld[g] == 0 ? 1 : mi.ld[g]);
        return u;
    }
    static size_t off_snap(const ModelInfo& mi, int64_t B) { return dev_wide_grad_layout(mi, B).total; }
    static size_t workspace_bytes(const ModelInfo& mi, int64_t B) {
        return off_snap(mi, B) + align256(units(mi) * (size_t)B * (sizeof(double2) << (2 * mi.n)));
    }
    static int refuse(const ModelInfo& mi, const qhea_device_noise* dn) {
        if (mi.n < 7 || mi.n > kDevWideMaxWires) return QHEA_EUNSUPPORTED;
        return device_log10_amplification(mi, dn, true) <= kMaxLog10AmplificationDevice ? QHEA_OK : QHEA_EUNSUPPORTED;
    }
    static int check(const qhea_model_desc* desc, const double* ham_diag, const qhea_device_noise* dn, int64_t count,
                     const double* trunk, std::initializer_list<const void*> required, void* workspace, void* stream,
                     NoisyCall& c) {
        return device_call_check({7, kDevWideMaxWires, false, false}, desc, ham_diag, dn, refuse, count, trunk, required, workspace,
                                 stream, c);
    }
    static int launch_bwd(const GradBatch& b, const qhea_device_noise* dn) {
        if (units(b.mi) == 0) return DevWideGradUnit::launch_bwd(b, dn);   // nothing to store: the inverse unit's launches
        const WideGradLayout L = wide_grad_layout(b.mi, b.batch);
        double* hv = reinterpret_cast<double*>(b.ws + L.off_hv);
        double* partial = reinterpret_cast<double*>(b.ws + L.off_partial);
        double2* rho = reinterpret_cast<double2*>(b.ws + L.off_rho);
        double2* obs = reinterpret_cast<double2*>(b.ws + L.off_obs);
        double2* snap = reinterpret_cast<double2*>(b.ws + off_snap(b.mi, b.bmax));
        const long nrec = (long)b.mi.sh.E + 3L * b.mi.n * b.mi.sh.blk;
        const DevWideGradCall c = call_record(b, dn, partial);
        return dispatch_wide_n(b.mi.n, [&](auto nn) {
            return launch_density_dev_wide_stored_grad<nn()>(c, hv, partial, rho, obs, snap, nrec, b.st);
        });
    }
};

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_device_noisy_wide_stored_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (batch < 0 || model_info(desc, mi) != QHEA_OK || mi.n < 7 || mi.n > kDevWideMaxWires) return 0;
    return DevWideStoredGradUnit::workspace_bytes(mi, batch);
}

int qhea_model_loss_grad_noisy_device_exact_wide_stored(const qhea_model_desc* desc, int64_t batch, const double* branch,
                                                        const double* trunk, const double* y, const double* params,
                                                        const double* ham_diag, const qhea_device_noise* dn,
                                                        double inv_batch_total, double* grad, double* pred, void* workspace,
                                                        size_t workspace_bytes, void* stream) {
    return grad_loss_grad<DevWideStoredGradUnit>(desc, batch, branch, trunk, y, params, ham_diag, dn, inv_batch_total, grad, pred,
                                                 workspace, workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_device_exact_wide_stored(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                                          const double* branch, const double* trunk, const double* y,
                                                          double* params, const double* ham_diag, const qhea_device_noise* dn,
                                                          const double* inv_batch_total, double* grad, int64_t grad_stride,
                                                          double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr,
                                                          double beta1, double beta2, double eps, double weight_decay,
                                                          void* workspace, size_t workspace_bytes, void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return grad_train_steps<DevWideStoredGradUnit>(desc, call, ham_diag, dn, lr);
}

}  // extern "C"
