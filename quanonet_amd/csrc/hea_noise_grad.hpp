// hea_noise_grad.hpp -- what the two sampled-trajectory gradient units share: hea_noise_grad.hip (n = 7..9, one wave per work
// item, qhea_model_*_noisy_wide) and hea_noise_grad_lds.hip (n = 10..12, one workgroup per work item, qhea_model_*_noisy_lds).
// A unit is its qubit range, its tile and the launch of its trajectory kernel (GradUnit); the kernels' argument record, the
// workspace layout, the checks and the bodies of the three entry points are here, the fold kernel's launcher is
// hea_noise_grad.hip's.  The contract is stated in include/quanonet_hea.h.
#pragma once
#include "hea_noise_traj.hpp"

namespace qhea {

// hea_density_grad.hip's reduce launch (weights, frequency chain rule, grad[P], grad[P + 1], Adam), as hea_density_grad.hpp
// declares it: that header's passes share names with hea_lds.hpp's, which the LDS unit includes
int launch_density_reduce(const qhea_model_desc* desc, const ModelInfo& mi, int64_t batch, const double* branch,
                          const double* trunk, const double* y, const double* rec, const double* pred, double inv_bt,
                          double* grad, const AdamArgs& adam, hipStream_t st);

struct NoisyGradArgs {
    NoiseArgs f;                            // the forward's record; f.tiles and f.partial are the unit's (tiles of its own size)
    const double* hd;                       // the readout-confused ham_diag, or NULL
    const double* w;                        // ansatz angles [blk, 3, n]
    int blk, width;                         // sub-layers; width = E + 3 n blk
    double* items;                          // [B * tiles][width]: d sum_t v / d x[e], then per (s, q) the (X, Y, Z) sums
    double* pred;                           // the caller's [B] or NULL
    double* pred_ws;                        // [B]
    double* rec;                            // [width][B]: d pred_b / d x[b, e], then d pred_b / d w[s, k, q]
};

// noisy_grad_fold_kernel (hea_noise_grad.hip) on `st`: a row's tiles added in tile order and divided by T -> pred and rec
int launch_noisy_grad_fold(const NoisyGradArgs& g, int n, int64_t batch, hipStream_t st);

// A unit: the qubit counts of its trajectory kernel, the trajectories per work item (part of the stated summation order) and the
// kernel's launch for g.f.B * g.f.tiles items
struct GradUnit {
    int nmin, nmax, tile;
    int (*launch)(int n, const NoisyGradArgs& g, hipStream_t st);
};

struct WideGradLayout { size_t off_gates, off_cs, off_part, off_mix, off_items, off_pred, off_rec, total; int tiles; long width; };
inline WideGradLayout wide_grad_layout(const GradUnit& u, const ModelInfo& mi, int64_t B, int64_t T) {
    WideGradLayout L{};
    L.tiles = (int)((T + u.tile - 1) / u.tile);
    L.width = mi.sh.E + 3L * mi.n * mi.sh.blk;
    const TableLayout t = table_layout(mi, B);
    L.off_gates = t.off_gates; L.off_cs = t.off_cs;
    size_t p = t.end;
    L.off_part = p;  p = align256(p + (size_t)B * L.tiles * sizeof(double2));
    L.off_mix = p;   p = align256(p + ((size_t)2 << mi.n) * sizeof(double));
    L.off_items = p; p = align256(p + (size_t)B * L.tiles * L.width * sizeof(double));
    L.off_pred = p;  p = align256(p + (size_t)B * sizeof(double));
    L.off_rec = p;   p = align256(p + (size_t)B * L.width * sizeof(double));
    L.total = p;
    return L;
}

inline size_t wide_grad_workspace_bytes(const GradUnit& u, const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise) {
    ModelInfo mi;
    const int64_t T = noise_values(noise);
    if (T < 1 || noise->shots > 0 || batch < 0 || model_info(desc, mi) != QHEA_OK || mi.n < u.nmin || mi.n > u.nmax) return 0;
    return wide_grad_layout(u, mi, batch, T).total;
}

// What opens both calls: noisy_call_check's order for a trajectory call at the unit's qubit counts, with shots > 0 refused as
// part of the noise setting (the gradient is of expectation mode)
inline int wide_grad_check(const GradUnit& u, const qhea_model_desc* desc, const double* ham_diag, const qhea_noise* noise,
                           int64_t row0, int64_t count, const double* trunk, std::initializer_list<const void*> required,
                           void* workspace, void* stream, NoisyCall& c) {
    ModelInfo mi;                                                        // (c.mi is noisy_call_check's to fill)
    const int rc = model_info(desc, mi);
    if (rc != QHEA_OK) return rc;
    if (noise_values(noise) < 1 || noise->shots > 0) return QHEA_EINVAL;
    return noisy_call_check({u.nmin, u.nmax, true, false}, desc, ham_diag, noise, row0, count, trunk, required, workspace, stream, c);
}

// The regions of a checked call's workspace, laid out once for its largest batch
struct WideGradCall {
    const GradUnit& u;
    const qhea_model_desc* desc; const ModelInfo& mi;
    WideGradLayout L;
    const double* ham_diag; const double* hd;       // hd: the mixed table (launched once per call), or NULL
    char* ws; hipStream_t st;
};

inline int wide_grad_open(const NoisyCall& c, int64_t bmax, const qhea_noise* noise, size_t workspace_bytes, WideGradCall& w) {
    w.L = wide_grad_layout(w.u, c.mi, bmax, c.T);
    if (!c.ws || workspace_bytes < w.L.total) return QHEA_EWORKSPACE;
    if (bmax * w.L.tiles > (int64_t)INT_MAX) return QHEA_EINVAL;         // one wave or workgroup per (row, tile)
    w.hd = nullptr;
    if (w.ham_diag)
        return launch_readout_mix(w.ham_diag, noise->readout, c.mi.n, reinterpret_cast<double*>(c.ws + w.L.off_mix), c.st, &w.hd);
    return QHEA_OK;
}

// The prep launch for one batch and the kernels' record from a call's layout (also the quantum-jump units', which set g.f.L and
// g.f.thr1 on top: hea_noise_jump_grad.hpp)
inline int wide_grad_prep(const qhea_model_desc* desc, const ModelInfo& mi, const WideGradLayout& L, char* ws, hipStream_t st,
                          const double* ham_diag, const double* hd, const qhea_noise* noise, int64_t T, int64_t row0, int64_t batch,
                          const double* branch, const double* trunk, const double* params, double* pred, NoisyGradArgs& g) {
    double4* gates = reinterpret_cast<double4*>(ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(ws + L.off_cs);
    const int rc = launch_prep_model(desc, mi, batch, branch, trunk, params, gates, cs, ws, st);
    if (rc != QHEA_OK) return rc;
    g.f = noise_args(desc, mi, noise, params, ham_diag, row0, batch, T);
    g.f.gates = gates; g.f.cs = cs; g.f.tiles = L.tiles;
    g.f.partial = reinterpret_cast<double2*>(ws + L.off_part);
    g.hd = hd; g.w = params + mi.off_ans; g.blk = (int)mi.sh.blk; g.width = (int)L.width;
    g.items = reinterpret_cast<double*>(ws + L.off_items);
    g.pred = pred; g.pred_ws = reinterpret_cast<double*>(ws + L.off_pred);
    g.rec = reinterpret_cast<double*>(ws + L.off_rec);
    return QHEA_OK;
}

// prep, trajectories, fold, reduce (+ Adam when adam.p) for one batch under `noise` (its seed: the step's)
inline int wide_grad_launch(const WideGradCall& w, const qhea_noise* noise, int64_t T, int64_t row0, int64_t batch,
                            const double* branch, const double* trunk, const double* y, const double* params, double inv_bt,
                            double* grad, double* pred, const AdamArgs& adam) {
    NoisyGradArgs g{};
    int rc = wide_grad_prep(w.desc, w.mi, w.L, w.ws, w.st, w.ham_diag, w.hd, noise, T, row0, batch, branch, trunk, params, pred, g);
    if (rc != QHEA_OK) return rc;
    rc = w.u.launch(w.mi.n, g, w.st);
    if (rc != QHEA_OK) return rc;
    rc = launch_noisy_grad_fold(g, w.mi.n, batch, w.st);
    if (rc != QHEA_OK) return rc;
    return launch_density_reduce(w.desc, w.mi, batch, branch, trunk, y, g.rec, g.pred_ws, inv_bt, grad, adam, w.st);
}

// qhea_model_loss_grad_noisy_wide / _lds
inline int wide_grad_loss_grad(const GradUnit& u, const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch,
                               const double* trunk, const double* y, const double* params, const double* ham_diag,
                               const qhea_noise* noise, double inv_batch_total, double* grad, double* pred, void* workspace,
                               size_t workspace_bytes, void* stream) {
    NoisyCall c;
    int rc = wide_grad_check(u, desc, ham_diag, noise, row0, batch, trunk, {branch, y, params, grad}, workspace, stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    WideGradCall w{u, desc, c.mi, {}, ham_diag, nullptr, c.ws, c.st};
    rc = wide_grad_open(c, batch, noise, workspace_bytes, w);
    if (rc != QHEA_OK) return rc;
    return wide_grad_launch(w, noise, c.T, row0, batch, branch, trunk, y, params, inv_batch_total, grad, pred, AdamArgs{});
}

// qhea_model_train_steps_noisy_wide / _lds
inline int wide_grad_train_steps(const GradUnit& u, const qhea_model_desc* desc, const TrainCall& call, const double* ham_diag,
                                 const qhea_noise* noise, double lr) {
    if (!desc || call.n_steps < 0 || call.first_step < 1) return QHEA_EINVAL;
    NoisyCall c;
    int rc = wide_grad_check(u, desc, ham_diag, noise, 0, call.n_steps, call.trunk,
                             {call.row_begin, call.inv_batch_total, call.branch, call.y, call.grad, call.params, call.exp_avg,
                              call.exp_avg_sq},
                             call.workspace, call.stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    const int64_t bmax = call_max_batch(call, c.mi.P, *desc);
    if (bmax < 0) return QHEA_EINVAL;
    WideGradCall w{u, desc, c.mi, {}, ham_diag, nullptr, c.ws, c.st};
    rc = wide_grad_open(c, bmax, noise, call.workspace_bytes, w);
    if (rc != QHEA_OK) return rc;
    for (int64_t i = 0; i < call.n_steps; ++i) {
        const StepView v = step_view(call, i, *desc);
        qhea_noise nz = *noise;
        nz.seed = noise->seed + (uint64_t)(call.first_step + i);         // fresh noise every step; a resumed run continues it
        rc = wide_grad_launch(w, &nz, c.T, v.r0, v.nb, v.branch, v.trunk, v.y, call.params, v.inv_bt, v.grad, nullptr,
                              adam_step(call, i, lr).adam);
        if (rc != QHEA_OK) return rc;
    }
    return QHEA_OK;
}

}  // namespace qhea
