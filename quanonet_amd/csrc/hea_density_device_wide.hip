// hea_density_device_wide.hip -- qhea_model_forward_noisy_device_exact_wide: the exact noisy forward under the calibrated device
// noise model (hea_density_device.hip) for n = 7, 8, 9, on the tiles of hea_density_wide.hip: rho of all rows of the call in the
// workspace, six wires at a time in 64 KiB of LDS, two stages per sub-layer (stage A the ring passes 0..4, stage B the passes
// 5..n-1), the same copy phases, pending-gate rule, grid and launch count.  tests/device_noise_reference.py restates the model
// in numpy, slot by slot.
//
// What a pass does is dev_ring_passes' of hea_density_device.hip: the pending gates of its wires with their kEnc / kRot sites,
// the CNOT of slot j with its two-qubit channel, the kTgt site of wire j and the kCtl site of wire (j + 1) mod n.  A stage's
// local wire is a global wire known at compile time: stage A the identity, stage B local 0, 1 -> global 0, 1 and local
// w >= 2 -> w + n - 6, so local pass LJ of stage B is slot LJ + n - 6 and the closing slot n - 1 the local pair (5, 0).
//
// The tables go to a stage in a by-value record of its own, DevStageArgs: the four sites of its six local wires and the
// two-qubit channel of its six local passes, 132 doubles, filled on the host per stage.  Every entry is indexed by compile-time
// constants only (the local wires of the pass, the site) and is a scalar of the launch, as hea_density_device.hip's header
// explains; a run-time index into a by-value record would put the record in scratch.  A ring stage reads up to 120 of them,
// more than a wave's scalar registers hold: as in density_dev_fwd_kernel the compiler loads them at entry and parks the overflow
// in lanes of vector registers (no memory, no scratch).  The record of all nine wires (198 doubles), built from the same text,
// gives the same vector and scalar register counts and occupancy in every stage kernel and a few more parked scalars (59
// against 50 in stage A); the per-stage record is also the shorter kernel argument and has one size for n = 7, 8, 9
// (profiles/r39_resource_usage.txt).
//
// The value tables take the asymmetric readout per bit, f = bit set ? r10[i] : r01[i], the loop over the bits unrolled so that
// the rates are scalars too; the read-out kernel is hea_density_wide.hpp's.  No workgroup waits on another, no atomics: a row's
// results are bitwise the same in any call.
#include "hea_density_device_wide_stages.hpp"

using namespace qhea;

extern "C" {

size_t qhea_model_device_exact_noisy_wide_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (batch < 0 || model_info(desc, mi) != QHEA_OK || mi.n < 7 || mi.n > kDevWideMaxWires) return 0;
    return wide_layout(mi, batch).total;
}

int qhea_model_forward_noisy_device_exact_wide(const qhea_model_desc* desc, int64_t batch, const double* branch,
                                               const double* trunk, const double* params, const double* ham_diag,
                                               const qhea_device_noise* dn, double* pred, double* shot_std, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    NoisyCall c;
    int rc = device_call_check({7, kDevWideMaxWires /* rho in the workspace, six wires at a time in LDS */, false, false}, desc,
                               ham_diag, dn, nullptr, batch, trunk, {branch, params, pred}, workspace, stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    const int n = c.mi.n;
    if (batch > (int64_t)INT_MAX >> (2 * (n - 6))) return QHEA_EINVAL;          // a stage has one workgroup per (row, tile)
    const WideLayout L = wide_layout(c.mi, batch);
    if (!workspace || workspace_bytes < L.total) return QHEA_EWORKSPACE;
    double4* gates = reinterpret_cast<double4*>(c.ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(c.ws + L.off_cs);
    double* hv = reinterpret_cast<double*>(c.ws + L.off_hv);
    double2* rho = reinterpret_cast<double2*>(c.ws + L.off_rho);
    rc = launch_prep_model(desc, c.mi, batch, branch, trunk, params, gates, cs, c.ws, c.st);
    if (rc != QHEA_OK) return rc;

    const WideDevSites sites(n, dn);
    DevWideCall w{};
    for (int stage = 0; stage < 2; ++stage) w.stage[stage] = stage_args(n, stage, sites, gates, cs, (int)c.mi.sh.E);
    w.out.bias = c.mi.has_bias ? params + c.mi.off_bias : nullptr;
    w.out.pred = pred; w.out.sd = shot_std;
    w.B = batch; w.pauli = desc->ham_pauli;
    for (int g = 0; g < 2; ++g) { w.nb[g] = c.mi.nb[g]; w.ld[g] = c.mi.ld[g]; }
    DevValueArgs v{};
    v.diag = ham_diag; v.off = desc->ham_offset; v.co = desc->ham_coeff;
    for (int q = 0; q < n; ++q) { v.r01[q] = dn->readout01[q]; v.r10[q] = dn->readout10[q]; }
    rc = dispatch_wide_n(n, [&](auto nn) {
        hipLaunchKernelGGL(density_dev_wide_values_kernel<nn()>, dim3(1), dim3(512), 0, c.st, v, hv);
        return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
    });
    if (rc != QHEA_OK) return rc;
    return dispatch_wide_n(n, [&](auto nn) { return launch_density_dev_wide<nn()>(w, rho, hv, c.st); });
}

}  // extern "C"
