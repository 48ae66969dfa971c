// hea_density_device_wide_grad.hpp -- what the two tiled gradient units under the calibrated device noise model share
// (hea_density_device_wide_grad.hip: the inverse walk; hea_density_device_wide_stored_grad.hip: the walk over stored states),
// n = 7, 8, 9: the workspace table and its kernel, the reverse ring and encoding passes on a tile, the inverse walk's two reverse
// stage kernels, its launch sequence and its unit record DevWideGradUnit.  hea_density_device_wide_grad.hip describes them.
// Everything sits in an unnamed namespace: each unit compiles its own copy, and a template nobody instantiates costs nothing.
#pragma once
#include "hea_density_device_grad.hpp"
#include "hea_density_device_wide_stages.hpp"
#include "hea_density_wide_grad.hpp"

namespace qhea {
namespace {

// ---- the table ----
constexpr int kWideTabStage = 6 * kTabWire, kWideTabDoubles = 2 * kWideTabStage;     // [stage][local wire] records
// what the host hands over per global wire q: [site][inverse, adjoint][5], then slot q's keep2, mix2, inverse keep2, inverse mix2
constexpr int kSrcSite = 10, kSrcSlot = 40, kSrcWire = 44;

struct DevWideTable { double v[kSrcWire * kDevWideMaxWires]; };

__global__ __launch_bounds__(64) void dev_wide_table_kernel(DevWideTable t, int n, double* out) {
    for (int i = threadIdx.x; i < kWideTabDoubles; i += 64) {
        const int stage = i / kWideTabStage, l = (i % kWideTabStage) / kTabWire, k = i % kTabWire;
        const int q = stage == 0 || l < 2 ? l : l + n - 6, j = stage == 0 ? l : l + n - 6;       // global wire, slot (both < n)
        double v = 0.0;
        if (k < kTabSlot) {
            const int site = k / kTabSite, form = (k % kTabSite) / 5, c = k % 5;
            if (form != kFormFwd) v = t.v[q * kSrcWire + site * kSrcSite + (form - 1) * 5 + c];
        } else if (k < kTabRead) {
            v = t.v[j * kSrcWire + kSrcSlot + (k - kTabSlot)];
        }
        out[i] = v;
    }
}

struct DevWideGradArgs {
    const double2* cs;                      // [B, E]
    const double* tab;                      // [kWideTabDoubles], written by dev_wide_table_kernel
    const double* w;                        // ansatz angles [blk, 3, n]
    long B;
    int E;
    double* rec;                            // the partials [E + 3 n blk][B][4^(n-6)]
};

// ---- reverse stages ----

// local wire L's pending gates of sub-layer s in reverse: the kRot site, the rotations, (the kEnc site, the encoding);
// tr[k] = this thread's share of d pred / d w[s, k, Q], tr[3] of d pred / d x[col + Q], Q the global wire
template <int N, int STAGE, int S, int L>
__device__ __forceinline__ void dev_wide_undo_wire(double2 (&e)[16], double2 (&o)[16], const DevWideGradArgs& a, const double* tab,
                                                   const double2* csr, int s, int col, bool enc, double* tr) {
    constexpr int Q = global_wire<N, STAGE>(L);
    undo_site<S>(e, o, tab, L, kRot);
    undo_rotations<N, S>(e, o, a.w, s, Q, tr);
    if (enc) dev_undo_encoding<S>(e, o, tab, L, csr[col + Q], tr);
}

// ring pass J of the circuit's n wires (slot J) in reverse, on the tile that holds both of its wires: the body of
// dev_ring_passes_back
template <int N, int J>
__device__ __forceinline__ void dev_wide_ring_pass_back(RowCtx<6>& cx, const DevWideGradArgs& a, const double2* csr, int s, int col,
                                                        bool enc) {
    constexpr int STAGE = J < 5 ? 0 : 1, LJ = J < 5 ? J : J - N + 6;
    using P = Pass<6, LJ>;
    static_assert(global_wire<N, STAGE>(P::t) == J && global_wire<N, STAGE>(P::c) == (J + 1) % N, "the pass serves slot J");
    const int i0 = P::base(cx.rank | opaque_zero()), b = i0 ^ fold(i0);
    const double* tab = a.tab + STAGE * kWideTabStage + opaque_szero();
    double2 e[16], o[16];
    P::load(e, cx.rho, b);
    P::load(o, cx.obs, b);
    undo_site<1>(e, o, tab, P::t, kTgt);
    undo_site<4>(e, o, tab, P::c, kCtl);
    const double* sl = tab + LJ * kTabWire + kTabSlot;
    undo_cnot2(e, uniform_load(sl + 2), uniform_load(sl + 3));
    undo_cnot2(o, uniform_load(sl), uniform_load(sl + 1));
    double tr[kTracesPerPass];
    int idx[kTracesPerPass];
#pragma unroll
    for (int i = 0; i < kTracesPerPass; ++i) { tr[i] = 0.0; idx[i] = -1; }
    const int ans = a.E + s * 3 * N;
    if (J <= N - 2) {
        constexpr int q = J + 1;
        dev_wide_undo_wire<N, STAGE, 4, P::c>(e, o, a, tab, csr, s, col, enc, tr);
        idx[0] = ans + q; idx[1] = ans + N + q; idx[2] = ans + 2 * N + q; idx[3] = enc ? col + q : -1;
    }
    if (J == 0) {
        dev_wide_undo_wire<N, STAGE, 1, P::t>(e, o, a, tab, csr, s, col, enc, tr + 4);
        idx[4] = ans; idx[5] = ans + N; idx[6] = ans + 2 * N; idx[7] = enc ? col : -1;
    }
    P::store(e, cx.rho, b);
    P::store(o, cx.obs, b);
    if (J <= N - 2) flush_traces<6>(cx, a, tr, idx);
    else __syncthreads();
}
template <int N, int J, int JEND>                                        // passes J, J - 1, .., JEND
__device__ __forceinline__ void dev_wide_ring_passes_back(RowCtx<6>& cx, const DevWideGradArgs& a, const double2* csr, int s,
                                                          int col, bool enc) {
    if constexpr (J >= JEND) {
        dev_wide_ring_pass_back<N, J>(cx, a, csr, s, col, enc);
        dev_wide_ring_passes_back<N, J - 1, JEND>(cx, a, csr, s, col, enc);
    }
}

// a reverse ring stage of sub-layer s: stage B passes n-1..5, stage A passes 4..0.  a.rec: the partials.  Grid: rows x 4^(n-6)
// workgroups, tile fastest
template <int N, int STAGE>
__global__ __launch_bounds__(kDensThreads) void density_dev_wide_ring_back_kernel(DevWideGradArgs a, double2* rho, double2* obs,
                                                                                  int s, int col, int enc) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    double2* rrow = rho + ((size_t)r << (2 * N));
    double2* orow = obs + ((size_t)r << (2 * N));
    const double2* csr = a.cs + r * a.E;
    RowCtx<6> cx = tile_ctx<N>(lds, tid, r, tile, a.B);
    tile_load<N, STAGE>(cx.rho, rrow, tile, tid, false);
    tile_load<N, STAGE>(cx.obs, orow, tile, tid, false);
    if (STAGE == 0) dev_wide_ring_passes_back<N, 4, 0>(cx, a, csr, s, col, enc != 0);
    else dev_wide_ring_passes_back<N, N - 1, 5>(cx, a, csr, s, col, enc != 0);
    tile_store<N, STAGE>(cx.rho, rrow, tile, tid);
    tile_store<N, STAGE>(cx.obs, orow, tile, tid);
}

// the local wires (LJ, LJ + 1) of a tile in reverse, those of them the stage serves (dev_wide_wire_pass' rule): a block's
// encoding -- kEnc site (inverse / adjoint), trace, RX^dagger
template <int N, int STAGE, int LJ>
__device__ __forceinline__ void dev_wide_wire_pass_back(RowCtx<6>& cx, const DevWideGradArgs& a, const double2* csr, int col) {
    constexpr int served = STAGE ? 12 - N : 0;                           // stage B: local wire >= 12 - n is global wire >= 6
    constexpr bool T = LJ >= served, C = LJ + 1 >= served;
    if constexpr (T || C) {
        using P = Pass<6, LJ>;
        const int i0 = P::base(cx.rank | opaque_zero()), b = i0 ^ fold(i0);
        const double* tab = a.tab + STAGE * kWideTabStage + opaque_szero();
        double2 e[16], o[16];
        P::load(e, cx.rho, b);
        P::load(o, cx.obs, b);
        double tr[kTracesPerPass];
        int idx[kTracesPerPass];
#pragma unroll
        for (int i = 0; i < kTracesPerPass; ++i) { tr[i] = 0.0; idx[i] = -1; }
        if (T) {
            constexpr int q = global_wire<N, STAGE>(LJ);
            dev_undo_encoding<1>(e, o, tab, LJ, csr[col + q], tr);
            idx[3] = col + q;
        }
        if (C) {
            constexpr int q = global_wire<N, STAGE>(LJ + 1);
            dev_undo_encoding<4>(e, o, tab, LJ + 1, csr[col + q], tr + 4);
            idx[7] = col + q;
        }
        P::store(e, cx.rho, b);
        P::store(o, cx.obs, b);
        flush_traces<6>(cx, a, tr, idx);
    }
}

// a reverse encoding stage: stage A wires 0..5, stage B wires 6..n-1
template <int N, int STAGE>
__global__ __launch_bounds__(kDensThreads) void density_dev_wide_enc_back_kernel(DevWideGradArgs a, double2* rho, double2* obs,
                                                                                 int col) {
    constexpr int TB = 2 * (N - 6);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];
    double2* lds = reinterpret_cast<double2*>(dens_lds);
    const int tid = threadIdx.x, tile = (int)(blockIdx.x & ((1u << TB) - 1));
    const long r = (long)(blockIdx.x >> TB);
    double2* rrow = rho + ((size_t)r << (2 * N));
    double2* orow = obs + ((size_t)r << (2 * N));
    const double2* csr = a.cs + r * a.E;
    RowCtx<6> cx = tile_ctx<N>(lds, tid, r, tile, a.B);
    tile_load<N, STAGE>(cx.rho, rrow, tile, tid, false);
    tile_load<N, STAGE>(cx.obs, orow, tile, tid, false);
    dev_wide_wire_pass_back<N, STAGE, 4>(cx, a, csr, col);
    dev_wide_wire_pass_back<N, STAGE, 2>(cx, a, csr, col);
    dev_wide_wire_pass_back<N, STAGE, 0>(cx, a, csr, col);
    tile_store<N, STAGE>(cx.rho, rrow, tile, tid);
    tile_store<N, STAGE>(cx.obs, orow, tile, tid);
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// the table's source for a checked setting whose channels are all invertible (fill_table of hea_density_device_grad.hip, per
// global wire, without the forward form and the readout)
void fill_wide_table(int n, const qhea_device_noise* dn, DevWideTable& t) {
    const WideDevSites sites(n, dn);
    for (double& v : t.v) v = 0.0;
    for (int q = 0; q < n; ++q) {
        double* w = t.v + q * kSrcWire;
        for (int k = 0; k < 4; ++k) {
            const Triple f = sites.at(k, q);
            double* inv = w + k * kSrcSite, * adj = inv + 5;
            element_form(Triple{1.0 / f.off, 1.0 / f.a, -f.b / f.a}, inv);
            element_form(f, adj);
            const double k01 = adj[2];                                   // the adjoint's weight matrix is the transposed one
            adj[2] = adj[3]; adj[3] = k01;
        }
        double* sl = w + kSrcSlot;
        slot_form(sites.lam2[q], sl[0], sl[1]);
        sl[2] = 1.0 / sl[0]; sl[3] = -sl[1] / sl[0];
    }
}

struct DevWideGradLayout { WideGradLayout wide; size_t off_tab, total; };

// wide_grad_layout's regions for `bmax` rows with the table behind them
DevWideGradLayout dev_wide_grad_layout(const ModelInfo& mi, int64_t bmax) {
    DevWideGradLayout L{};
    L.wide = wide_grad_layout(mi, bmax);
    L.off_tab = L.wide.total;
    L.total = align256(L.off_tab + kWideTabDoubles * sizeof(double));
    return L;
}

// what one batch's launches read
struct DevWideGradCall {
    DevWideCall fwd;                        // the forward sweep; fwd.out.pred: pred in the workspace
    DevValueArgs values;
    DevWideGradArgs bwd;                    // bwd.rec: the partials
    DensGradArgs basis;                     // what the dagger-of-basis stages read: f.cs, f.E, f.B
    double* rec;                            // [E + 3 n blk][B]
    double* pred;                           // the caller's pred or NULL
};

// every launch of one batch between the prep kernel and the reduce kernel, in stream order
template <int N>
int launch_density_dev_wide_grad(const DevWideGradCall& c, double* hv, double* partial, double2* rho, double2* obs, long nrec,
                                 hipStream_t st) {
    constexpr int tiles = 1 << (2 * (N - 6));
    const long B = c.bwd.B;
    const dim3 grid((unsigned)(B << (2 * (N - 6)))), block(kDensThreads);
    hipLaunchKernelGGL(density_dev_wide_values_kernel<N>, dim3(1), dim3(512), 0, st, c.values, hv);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    int rc = launch_density_dev_wide<N>(c.fwd, rho, hv, st);
    if (rc != QHEA_OK) return rc;
    hipLaunchKernelGGL(density_wide_observable_kernel<N>, grid, block, 0, st, hv, obs);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    if (c.fwd.pauli != QHEA_PAULI_Z) {
        const int kind = c.fwd.pauli == QHEA_PAULI_X ? 3 : 4;
        rc = launch_dynamic_lds(density_wide_wires_back_kernel<N, 1, true>, grid, block, kWideBwdLds, st, c.basis, rho, obs, 0, kind);
        if (rc == QHEA_OK)
            rc = launch_dynamic_lds(density_wide_wires_back_kernel<N, 0, true>, grid, block, kWideBwdLds, st, c.basis, rho, obs, 0,
                                    kind);
        if (rc != QHEA_OK) return rc;
    }
    const DevWideGradArgs& a = c.bwd;
    int s = c.fwd.nb[0] * c.fwd.ld[0] + c.fwd.nb[1] * c.fwd.ld[1], col = N * (c.fwd.nb[0] + c.fwd.nb[1]);
    for (int g = 1; g >= 0; --g) {
        for (int b = c.fwd.nb[g] - 1; b >= 0; --b) {
            col -= N;
            for (int l = c.fwd.ld[g] - 1; l >= 0; --l) {
                --s;
                rc = launch_dynamic_lds(density_dev_wide_ring_back_kernel<N, 1>, grid, block, kWideBwdLds, st, a, rho, obs, s, col,
                                        (int)(l == 0));
                if (rc == QHEA_OK)
                    rc = launch_dynamic_lds(density_dev_wide_ring_back_kernel<N, 0>, grid, block, kWideBwdLds, st, a, rho, obs, s,
                                            col, (int)(l == 0));
                if (rc != QHEA_OK) return rc;
            }
            if (c.fwd.ld[g] == 0) {
                rc = launch_dynamic_lds(density_dev_wide_enc_back_kernel<N, 1>, grid, block, kWideBwdLds, st, a, rho, obs, col);
                if (rc == QHEA_OK)
                    rc = launch_dynamic_lds(density_dev_wide_enc_back_kernel<N, 0>, grid, block, kWideBwdLds, st, a, rho, obs, col);
                if (rc != QHEA_OK) return rc;
            }
        }
    }
    const long nsum = nrec * B, nthr = nsum > B ? nsum : B;
    hipLaunchKernelGGL(density_wide_fold_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, partial, c.rec, nsum, tiles,
                       c.fwd.out.pred, c.pred, B);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

// The unit record of grad_loss_grad / grad_train_steps (hea_density_grad.hpp): the channel sites of a qhea_device_noise on tiles
struct DevWideGradUnit {
    using Noise = qhea_device_noise;
    static constexpr bool kStepCheckFirst = false;                       // as DevGradUnit: see the header comment
    static size_t workspace_bytes(const ModelInfo& mi, int64_t B) { return dev_wide_grad_layout(mi, B).total; }
    // QHEA_EUNSUPPORTED outside n = 7..9 and for what the guard refuses, between the setting's checks and the shared ones
    static int refuse(const ModelInfo& mi, const qhea_device_noise* dn) {
        if (mi.n < 7 || mi.n > kDevWideMaxWires) return QHEA_EUNSUPPORTED;
        return device_log10_amplification(mi, dn) <= kMaxLog10AmplificationDevice ? QHEA_OK : QHEA_EUNSUPPORTED;
    }
    static int check(const qhea_model_desc* desc, const double* ham_diag, const qhea_device_noise* dn, int64_t count,
                     const double* trunk, std::initializer_list<const void*> required, void* workspace, void* stream,
                     NoisyCall& c) {
        return device_call_check({7, kDevWideMaxWires /* rho and O in the workspace, six wires at a time in LDS */, false, false},
                                 desc, ham_diag, dn, refuse, count, trunk, required, workspace, stream, c);
    }
    // a stage has one workgroup per (row, tile)
    static bool batch_ok(const ModelInfo& mi, int64_t B) { return B <= (int64_t)INT_MAX >> (2 * (mi.n - 6)); }
    // the table, at its offset in a workspace for `bmax` rows
    static int once(const ModelInfo& mi, const qhea_device_noise* dn, char* ws, int64_t bmax, hipStream_t st) {
        DevWideTable t;
        fill_wide_table(mi.n, dn, t);
        hipLaunchKernelGGL(dev_wide_table_kernel, dim3(1), dim3(64), 0, st, t, mi.n,
                           reinterpret_cast<double*>(ws + dev_wide_grad_layout(mi, bmax).off_tab));
        return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
    }
    // what one batch's launches read; `partial`: where the reverse stages write
    static DevWideGradCall call_record(const GradBatch& b, const qhea_device_noise* dn, double* partial) {
        const int n = b.mi.n;
        DevWideGradCall c{};
        const WideDevSites sites(n, dn);
        for (int stage = 0; stage < 2; ++stage) c.fwd.stage[stage] = stage_args(n, stage, sites, b.gates, b.cs, (int)b.mi.sh.E);
        c.fwd.out.bias = b.mi.has_bias ? b.params + b.mi.off_bias : nullptr;
        c.fwd.out.pred = b.pred_ws; c.fwd.out.sd = nullptr;
        c.fwd.B = b.batch; c.fwd.pauli = b.desc->ham_pauli;
        for (int g = 0; g < 2; ++g) { c.fwd.nb[g] = b.mi.nb[g]; c.fwd.ld[g] = b.mi.ld[g]; }
        c.values.diag = b.ham_diag; c.values.off = b.desc->ham_offset; c.values.co = b.desc->ham_coeff;
        for (int q = 0; q < n; ++q) { c.values.r01[q] = dn->readout01[q]; c.values.r10[q] = dn->readout10[q]; }
        c.bwd.cs = b.cs;
        c.bwd.tab = reinterpret_cast<const double*>(b.ws + dev_wide_grad_layout(b.mi, b.bmax).off_tab);
        c.bwd.w = b.params + b.mi.off_ans;
        c.bwd.B = b.batch; c.bwd.E = (int)b.mi.sh.E; c.bwd.rec = partial;
        c.basis.f.cs = b.cs; c.basis.f.E = (int)b.mi.sh.E; c.basis.f.B = b.batch;
        c.rec = b.rec; c.pred = b.pred;
        return c;
    }
    static int launch_bwd(const GradBatch& b, const qhea_device_noise* dn) {
        const WideGradLayout L = wide_grad_layout(b.mi, b.batch);
        double* hv = reinterpret_cast<double*>(b.ws + L.off_hv);
        double* partial = reinterpret_cast<double*>(b.ws + L.off_partial);
        double2* rho = reinterpret_cast<double2*>(b.ws + L.off_rho);
        double2* obs = reinterpret_cast<double2*>(b.ws + L.off_obs);
        const long nrec = (long)b.mi.sh.E + 3L * b.mi.n * b.mi.sh.blk;
        const DevWideGradCall c = call_record(b, dn, partial);
        return dispatch_wide_n(b.mi.n, [&](auto nn) { return launch_density_dev_wide_grad<nn()>(c, hv, partial, rho, obs, nrec, b.st); });
    }
};

}  // namespace
}  // namespace qhea
