// hea_noise_jump_grad.hpp -- what the two quantum-jump gradient units share beyond hea_noise_jump.hpp and hea_noise_grad.hpp:
// hea_noise_device_grad.hip (n = 7..9, one wave per work item, qhea_model_*_noisy_device) and hea_noise_device_grad_lds.hip
// (n = 10..12, one workgroup per work item, qhea_model_*_noisy_device_lds).  The fenced read of a site's 1 / sqrt(1 - gamma)
// for the way back, the host's fill of that table, and the whole host side of the calls: the checks that open them, the
// workspace layout and query, the call record, open (table and h', once per call), launch (prep, trajectories, fold, reduce) and
// the bodies of loss_grad and train_steps.  A unit hands them a struct of static members U:
//   Table, Args, Snap      the table's type, the kernel's record (tab, words, snap, words_stride, snap_stride) and the element
//                          type of a snapshot
//   unit                   its GradUnit (qubit range, tile)
//   jump(tb)               the JumpTable / WideDevTable part of a Table
//   cap(n)                 residents of a launch at most; a launch has min(items, cap) and the workspace holds as many areas
//   words_stride(segs), snap_stride(blocks, n)     elements per resident
//   launch_tables(...), launch(n, g, d, residents, st)     the tables kernel and the trajectory kernel
// The kernels' record (NoisyGradArgs) is filled by hea_noise_grad.hpp's wide_grad_prep.  The contract is stated in
// include/quanonet_hea.h.
#pragma once
#include <climits>
#include <initializer_list>

#include "hea_noise_jump.hpp"
#include "hea_noise_grad.hpp"

namespace qhea {
namespace {

// 1 / sqrt(1 - gamma) of a site from a table with inv[4][W], read where the site uses it (site_pair's fence)
template <class Tab>
__device__ __forceinline__ double site_inv(const Tab* __restrict__ tab, int site, int q) {
    int fence = 0;
    asm volatile("" : "+s"(fence));
    return (&tab->inv[site][q])[fence];
}

// inv[site][q] = 1 / gs[site][q][1] for the n wires of a filled table
template <class Inv, class Gs>
inline void fill_site_inv(int n, const Gs& gs, Inv& inv) {
    for (int site = 0; site < 4; ++site)
        for (int q = 0; q < n; ++q) inv[site][q] = 1.0 / gs[site][q][1];
}

// the checks of qhea_model_forward_noisy_device in its order, shots != 0 refused with the sampling record, then the site that
// cannot be walked back (1 - gamma == 0)
inline int device_grad_check(const GradUnit& u, const qhea_model_desc* desc, const double* ham_diag, const qhea_device_noise* dn,
                             const qhea_sampling* sampling, int64_t row0, int64_t count, const double* trunk,
                             std::initializer_list<const void*> required, void* workspace, void* stream, NoisyCall& c, qhea_noise& nz) {
    ModelInfo probe;
    int rc = model_info(desc, probe);
    if (rc != QHEA_OK) return rc;
    rc = device_noise_check(probe.n, dn);
    if (rc != QHEA_OK) return rc;
    if (!sampling || sampling->shots != 0) return QHEA_EINVAL;
    nz = sampling_as_noise(sampling);
    rc = noisy_call_check({u.nmin, u.nmax, true, false}, desc, ham_diag, &nz, row0, count, trunk, required, workspace, stream, c);
    if (rc != QHEA_OK) return rc;
    int site, wire;
    if (qhea_device_noise_singular_site(probe.n, dn, &site, &wire) == 1) return QHEA_EINVAL;
    return QHEA_OK;
}

// hea_noise_grad.hpp's layout, then the table, the segments' words and the snapshots of min(items, U::cap) residents: a function
// of the shape, the batch and T only
struct JumpGradLayout { WideGradLayout w; size_t off_tab, off_words, off_snap, total; long words_stride, snap_stride; };
template <class U>
inline int jump_grad_residents(int n, int64_t items) {
    const int cap = U::cap(n);
    return (int)(items < cap ? items : cap);
}
template <class U>
inline JumpGradLayout jump_grad_layout(const ModelInfo& mi, int64_t B, int64_t T) {
    JumpGradLayout L{};
    L.w = wide_grad_layout(U::unit, mi, B, T);
    const int res = jump_grad_residents<U>(mi.n, B * L.w.tiles);
    const long blocks = mi.nb[0] + mi.nb[1];
    L.words_stride = U::words_stride(blocks + mi.sh.blk);
    L.snap_stride = U::snap_stride(blocks, mi.n);
    size_t p = L.w.total;
    L.off_tab = p;   p = align256(p + sizeof(typename U::Table));
    L.off_words = p; p = align256(p + (size_t)res * L.words_stride * sizeof(unsigned));
    L.off_snap = p;  p = align256(p + (size_t)res * L.snap_stride * sizeof(typename U::Snap));
    L.total = p;
    return L;
}

// the workspace query of both units: 0 for a record the calls refuse
template <class U>
inline size_t jump_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling) {
    if (!sampling || sampling->shots != 0) return 0;
    const qhea_noise nz = sampling_as_noise(sampling);
    ModelInfo mi;
    const int64_t T = noise_values(&nz);
    if (T < 1 || batch < 0 || model_info(desc, mi) != QHEA_OK || mi.n < U::unit.nmin || mi.n > U::unit.nmax) return 0;
    return jump_grad_layout<U>(mi, batch, T).total;
}

// The regions of a checked call's workspace, laid out once for its largest batch, and the host's copy of the table
template <class U>
struct JumpGradCall {
    const qhea_model_desc* desc; const ModelInfo& mi;
    JumpGradLayout L;
    const double* ham_diag; const double* hd;
    typename U::Table tb; bool any;
    char* ws; hipStream_t st;
};

// layout for the call's largest batch, and the once-per-call launch: the table and h'
template <class U>
inline int jump_grad_open(const NoisyCall& c, int64_t bmax, const qhea_device_noise* dn, size_t workspace_bytes, JumpGradCall<U>& w) {
    w.L = jump_grad_layout<U>(c.mi, bmax, c.T);
    if (!c.ws || workspace_bytes < w.L.total) return QHEA_EWORKSPACE;
    if (bmax * w.L.w.tiles > (int64_t)INT_MAX) return QHEA_EINVAL;       // one wave or workgroup per (row, tile)
    const int n = c.mi.n;
    w.tb = typename U::Table{};
    auto& t = U::jump(w.tb);
    fill_jump_table(n, dn, t, w.any);
    fill_site_inv(n, t.gs, w.tb.inv);
    t.off = w.desc->ham_offset; t.co = w.desc->ham_coeff; t.diag = w.ham_diag;
    t.L = jump_calls(n, c.mi.nb, c.mi.ld); t.pauli = (unsigned)w.desc->ham_pauli;
    double* mix = reinterpret_cast<double*>(c.ws + w.L.w.off_mix);
    U::launch_tables(w.tb, reinterpret_cast<typename U::Table*>(c.ws + w.L.off_tab), w.ham_diag, w.desc->ham_coeff, n, mix, c.st);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    w.hd = mix + ((size_t)((n - 1) & 1) << n);
    return QHEA_OK;
}

// prep, trajectories, fold, reduce (+ Adam when adam.p) for one batch under the stream key `nz.seed`
template <class U>
inline int jump_grad_launch(const JumpGradCall<U>& w, const qhea_noise& nz, int64_t T, int64_t row0, int64_t batch,
                            const double* branch, const double* trunk, const double* y, const double* params, double inv_bt,
                            double* grad, double* pred, const AdamArgs& adam) {
    NoisyGradArgs g{};
    int rc = wide_grad_prep(w.desc, w.mi, w.L.w, w.ws, w.st, w.ham_diag, w.hd, &nz, T, row0, batch, branch, trunk, params, pred, g);
    if (rc != QHEA_OK) return rc;
    g.f.L = U::jump(w.tb).L;
    g.f.thr1 = w.any ? 1 : 0;                                            // an ideal setting draws nothing
    typename U::Args d{};
    d.tab = reinterpret_cast<const typename U::Table*>(w.ws + w.L.off_tab);
    d.words = reinterpret_cast<unsigned*>(w.ws + w.L.off_words);
    d.snap = reinterpret_cast<typename U::Snap*>(w.ws + w.L.off_snap);
    d.words_stride = w.L.words_stride; d.snap_stride = w.L.snap_stride;
    rc = U::launch(w.mi.n, g, d, jump_grad_residents<U>(w.mi.n, batch * w.L.w.tiles), w.st);
    if (rc != QHEA_OK) return rc;
    rc = launch_noisy_grad_fold(g, w.mi.n, batch, w.st);
    if (rc != QHEA_OK) return rc;
    return launch_density_reduce(w.desc, w.mi, batch, branch, trunk, y, g.rec, g.pred_ws, inv_bt, grad, adam, w.st);
}

// qhea_model_loss_grad_noisy_device / _lds
template <class U>
inline int jump_grad_loss_grad(const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch, const double* trunk,
                               const double* y, const double* params, const double* ham_diag, const qhea_device_noise* dn,
                               const qhea_sampling* sampling, double inv_batch_total, double* grad, double* pred, void* workspace,
                               size_t workspace_bytes, void* stream) {
    NoisyCall c;
    qhea_noise nz{};
    int rc = device_grad_check(U::unit, desc, ham_diag, dn, sampling, row0, batch, trunk, {branch, y, params, grad}, workspace, stream,
                               c, nz);
    if (rc != QHEA_OK || c.empty) return rc;
    JumpGradCall<U> w{desc, c.mi, {}, ham_diag, nullptr, {}, false, c.ws, c.st};
    rc = jump_grad_open(c, batch, dn, workspace_bytes, w);
    if (rc != QHEA_OK) return rc;
    return jump_grad_launch(w, nz, c.T, row0, batch, branch, trunk, y, params, inv_batch_total, grad, pred, AdamArgs{});
}

// qhea_model_train_steps_noisy_device / _lds
template <class U>
inline int jump_grad_train_steps(const qhea_model_desc* desc, const TrainCall& call, const double* ham_diag,
                                 const qhea_device_noise* dn, const qhea_sampling* sampling, double lr) {
    if (!desc || call.n_steps < 0 || call.first_step < 1) return QHEA_EINVAL;
    NoisyCall c;
    qhea_noise nz{};
    int rc = device_grad_check(U::unit, desc, ham_diag, dn, sampling, 0, call.n_steps, call.trunk,
                               {call.row_begin, call.inv_batch_total, call.branch, call.y, call.grad, call.params, call.exp_avg,
                                call.exp_avg_sq},
                               call.workspace, call.stream, c, nz);
    if (rc != QHEA_OK || c.empty) return rc;
    const int64_t bmax = call_max_batch(call, c.mi.P, *desc);
    if (bmax < 0) return QHEA_EINVAL;
    JumpGradCall<U> w{desc, c.mi, {}, ham_diag, nullptr, {}, false, c.ws, c.st};
    rc = jump_grad_open(c, bmax, dn, call.workspace_bytes, w);
    if (rc != QHEA_OK) return rc;
    for (int64_t i = 0; i < call.n_steps; ++i) {
        const StepView v = step_view(call, i, *desc);
        qhea_noise step = nz;
        step.seed = nz.seed + (uint64_t)(call.first_step + i);           // fresh draws every step; a resumed run continues them
        rc = jump_grad_launch(w, step, c.T, v.r0, v.nb, v.branch, v.trunk, v.y, call.params, v.inv_bt, v.grad, nullptr,
                              adam_step(call, i, lr).adam);
        if (rc != QHEA_OK) return rc;
    }
    return QHEA_OK;
}

}  // namespace
}  // namespace qhea
