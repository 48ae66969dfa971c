// hea_density_wide.hip -- qhea_model_forward_noisy_exact_wide: the exact noisy forward of hea_density.hip for n = 7, 8, 9, where
// a row's 4^n elements of rho (256 KiB, 1 MiB, 4 MiB) no longer fit in LDS.  rho of all rows of the call lives in the workspace,
// 4^n x 16 bytes per row, in hea_density.hip's index layout (bit 2q: wire q's row bit, bit 2q + 1: its column bit).
//
// A stage is one launch over rows x tiles.  A tile is the 4^6 elements that share the 2 (n - 6) index bits of the wires a stage
// leaves alone; a workgroup of 256 threads copies its tile into 64 KiB of LDS (the n = 6 slot layout and fold), runs passes of
// Pass<6, J> over it (16 elements per thread, one barrier per pass) and copies it back.  Two tilings serve every pass:
//   stage A: local wires (0, 1, 2, 3, 4, 5).  element i = tile << 12 | l: one contiguous 64 KiB block of the row.
//   stage B: local wires (0, 1, n-4, n-3, n-2, n-1).  element i = (l & 15) | tile << 4 | (l >> 4) << (2n - 8): runs of 16
//            contiguous elements (256 bytes).
// A sub-layer is stage A with the ring passes j = 0..4 (Pass<6, j>), then stage B with j = 5..n-1: the pair (j, j + 1) is the
// local pair (j - n + 6, j - n + 7) and the closing pair (n - 1, 0) the local pair (5, 0), Pass<6, j - n + 6>.  The pending-gate
// rule is hea_density.hip's in global wires: pass 0 applies wire 0's gates, every pass j <= n - 2 wire j + 1's, pass n - 1 none.
// Blocks without sub-layers and the basis change of the X / Y read-outs are one-qubit stages on the same tiles: stage A serves
// wires 0..5, stage B wires 6..n-1 only.  The first stage of a circuit loads nothing: tile 0 starts from |0><0|, the others
// from zero.
//
// The launch boundary is the only synchronisation between the tiles of a row: no workgroup waits on another, stream order
// carries a stage's stores to the next.  The copy between global memory and LDS is a phase of its own in which consecutive
// lanes take consecutive elements of a run.
//
// Read-out: one small kernel per call writes h'[2^n] and h2'[2^n] (the value table and its square under the readout
// confusion, n two-point mixes) to the workspace; a wave per row adds p_k h'[k] and p_k h2'[k] over diag rho: lane l the terms
// k = l + 64 r in the order r = 0, 1, .., then the 64 lane sums by the xor butterfly, offsets 32, 16, .. 1.  No atomics, nothing
// depends on the batch or on other rows: a row's results are bitwise the same in any call.
//
// The tile maps, the copy phase, the read-out kernel, the workspace layout and the dispatch on n are hea_density_wide.hpp's,
// shared with hea_density_device_wide.hip (the same stages under a calibrated device noise model).  The stage kernels, the value
// table kernel and the launch sequence are hea_density_wide_stages.hpp's, shared with hea_density_wide_grad.hip (whose forward
// sweep they are).
#include "hea_density_wide_stages.hpp"

using namespace qhea;

extern "C" {

size_t qhea_model_exact_noisy_wide_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (batch < 0 || model_info(desc, mi) != QHEA_OK || mi.n < 7 || mi.n > 9) return 0;
    return wide_layout(mi, batch).total;
}

int qhea_model_forward_noisy_exact_wide(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                                        const double* params, const double* ham_diag, const qhea_noise* noise, double* pred,
                                        double* shot_std, void* workspace, size_t workspace_bytes, void* stream) {
    NoisyCall c;
    int rc = noisy_call_check({7, 9 /* rho in the workspace, six wires at a time in LDS */, false, false}, desc, ham_diag, noise,
                              0, batch, trunk, {branch, params, pred}, workspace, stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    if (batch > (int64_t)INT_MAX >> (2 * (c.mi.n - 6))) return QHEA_EINVAL;     // a stage has one workgroup per (row, tile)
    const WideLayout L = wide_layout(c.mi, batch);
    if (!workspace || workspace_bytes < L.total) return QHEA_EWORKSPACE;
    double4* gates = reinterpret_cast<double4*>(c.ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(c.ws + L.off_cs);
    double* hv = reinterpret_cast<double*>(c.ws + L.off_hv);
    double2* rho = reinterpret_cast<double2*>(c.ws + L.off_rho);
    rc = launch_prep_model(desc, c.mi, batch, branch, trunk, params, gates, cs, c.ws, c.st);
    if (rc != QHEA_OK) return rc;

    DensArgs a = dens_args(desc, c.mi, noise, params, ham_diag, batch, gates, cs);
    a.pred = pred; a.sd = shot_std;
    hipLaunchKernelGGL(density_wide_values_kernel, dim3(1), dim3(512), 0, c.st, a, c.mi.n, hv);
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    return dispatch_wide_n(c.mi.n, [&](auto n) { return launch_density_wide<n()>(a, rho, hv, c.st); });
}

}  // extern "C"
