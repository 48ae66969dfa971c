// hea_noise_jump_grad.hpp -- what the two quantum-jump gradient units share beyond hea_noise_jump.hpp and hea_noise_grad.hpp:
// hea_noise_device_grad.hip (n = 7..9, one wave per work item, qhea_model_*_noisy_device) and hea_noise_device_grad_lds.hip
// (n = 10..12, one workgroup per work item, qhea_model_*_noisy_device_lds).  The fenced read of a site's 1 / sqrt(1 - gamma)
// for the way back, the host's fill of that table, and the checks that open both units' calls.  The contract is stated in
// include/quanonet_hea.h.
#pragma once
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

// the workspace query of both units: 0 for a record the calls refuse
template <class Layout>
inline size_t device_grad_workspace_bytes(const GradUnit& u, Layout layout, const qhea_model_desc* desc, int64_t batch,
                                          const qhea_sampling* sampling) {
    if (!sampling || sampling->shots != 0) return 0;
    const qhea_noise nz = sampling_as_noise(sampling);
    ModelInfo mi;
    const int64_t T = noise_values(&nz);
    if (T < 1 || batch < 0 || model_info(desc, mi) != QHEA_OK || mi.n < u.nmin || mi.n > u.nmax) return 0;
    return layout(mi, batch, T).total;
}

}  // namespace
}  // namespace qhea
