// hea_density_device_wide_grad.hip -- qhea_model_loss_grad_noisy_device_exact_wide / qhea_model_train_steps_noisy_device_exact_wide:
// the MSE loss of the exact noisy forward under the calibrated device noise model and its exact gradient (the quantity and the
// inverse walk of hea_density_device_grad.hip) for n = 7, 8, 9, on the tiles of hea_density_wide_grad.hip.  rho and the
// observable O of all rows of the call live in the workspace, 4^n x 16 bytes per row each.
//
// Forward sweep: the value-table kernel, the stage launches and the read-out kernel of hea_density_device_wide_stages.hpp, word
// for word, so a row's pred is what qhea_model_forward_noisy_device_exact_wide returns for it.  O_N, the dagger-of-basis stages,
// the per-tile trace partials and the fold launch are hea_density_wide_grad.hpp's: under a device model h' comes from the
// asymmetric values kernel and nothing else changes.
//
// Reverse stages: a reverse sub-layer is stage B with the ring passes j = n-1..5, then stage A with j = 4..0, each one launch
// over rows x 4^(n-6) workgroups of 256 threads with the tiles of rho and O in 2 x 64 KiB of LDS.  A pass is the body of
// dev_ring_passes_back on the local pass Pass<6, j < 5 ? j : j - n + 6>, in global wires through global_wire<N, STAGE>:
//   1. the kTgt site of wire j and the kCtl site of wire (j + 1) mod n: inverse form on rho, adjoint form on O;
//   2. D2 of slot j (the slot's inverse pair on rho, its forward pair on O) and the CNOT, both inside undo_cnot2;
//   3. per pending wire (pass 0: wire 0; every pass j <= n - 2: wire j + 1): the kRot site, the three traces with their
//      un-rotations, and in a block's first sub-layer the kEnc site, its trace and RX^dagger.
// The closing slot n - 1 is the local pair (5, 0) of stage B and has no pending wire.  A block without sub-layers is the reverse
// of dev_wide_wire_pass with kind 0, stage B (wires 6..n-1) then stage A (wires 0..5).
//
// Constants.  The reverse stages of the uniform unit already take every vector register, and a reverse ring pass needs four
// sites in two forms of five doubles plus four slot factors: by-value arguments would be parked in vector registers the walk
// has none left of (hea_density_device_grad.hip met the same wall).  So the constants sit in the workspace, as a table of
// [stage][local wire] records in that unit's layout of one wire (kTabWire doubles: [site][form][5], then the four D2 factors
// of the local pass of that index), so that every index is a compile-time constant of the pass and undo_site is shared.  The
// host composes the two forms of every site and the four factors of every slot per global wire (kSrcWire doubles each, 396 for
// nine wires: what fits a kernel argument); dev_wide_table_kernel, one workgroup launched once per call, places them at their
// local indices (stage A: local = global; stage B: local 0, 1 = global 0, 1, local l >= 2 = global l + n - 6; local pass LJ is
// slot LJ or LJ + n - 6).  The forward form's entries and the readout entries of a record stay zero: the forward stages keep
// their by-value DevStageArgs, the values kernel its DevValueArgs.  The reverse stages read a site's constants where they use
// them, through uniform_load behind opaque_szero().
//
// kStepCheckFirst = false: train_steps reports first_step < 1 after the unit's checks, where the n <= 6 device unit
// (DevGradUnit) reports it, not ahead of them as the uniform units do.
//
// No atomics, no flags, no spinning, no grid barrier: the launch boundary is the only synchronisation between workgroups, and
// a row's pred and records are bitwise independent of the batch, the grid and the chunking.
#include "hea_density_device_wide_grad.hpp"

using namespace qhea;

extern "C" {

size_t qhea_model_device_noisy_wide_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (batch < 0 || model_info(desc, mi) != QHEA_OK || mi.n < 7 || mi.n > kDevWideMaxWires) return 0;
    return DevWideGradUnit::workspace_bytes(mi, batch);
}

int qhea_model_loss_grad_noisy_device_exact_wide(const qhea_model_desc* desc, int64_t batch, const double* branch,
                                                 const double* trunk, const double* y, const double* params,
                                                 const double* ham_diag, const qhea_device_noise* dn, double inv_batch_total,
                                                 double* grad, double* pred, void* workspace, size_t workspace_bytes,
                                                 void* stream) {
    return grad_loss_grad<DevWideGradUnit>(desc, batch, branch, trunk, y, params, ham_diag, dn, inv_batch_total, grad, pred,
                                           workspace, workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_device_exact_wide(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                                   const double* branch, const double* trunk, const double* y, double* params,
                                                   const double* ham_diag, const qhea_device_noise* dn,
                                                   const double* inv_batch_total, double* grad, int64_t grad_stride,
                                                   double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                                                   double beta2, double eps, double weight_decay, void* workspace,
                                                   size_t workspace_bytes, void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return grad_train_steps<DevWideGradUnit>(desc, call, ham_diag, dn, lr);
}

}  // extern "C"
