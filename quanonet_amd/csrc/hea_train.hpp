// hea_train.hpp -- host side shared by the entry points that run a schedule of training steps (hea_api.hip,
// hea_density_grad.hip): the call record, the step's Adam arguments, the schedule and member-record checks.  No device code.
#pragma once
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "hea_adam.hpp"
#include "../../include/quanonet_hea.h"

namespace qhea {

// What every train-steps entry point is given besides its model(s): filled once by the extern "C" function, read by whatever
// runs the steps.  Member calls: member 0's pointers, the other members' a MemberStride further.
struct TrainCall {
    int64_t n_steps; const int64_t* row_begin;                      // step i trains on rows row_begin[i] .. row_begin[i + 1]
    const double* branch; const double* trunk; const double* y;
    double* params;
    const double* inv_batch_total;                                  // [n_steps]
    double* grad; int64_t grad_stride;                              // step i's [grads | sse | sum y^2] row
    double* exp_avg; double* exp_avg_sq;
    int64_t first_step;                                             // Adam step number of step 0 (>= 1)
    double beta1, beta2, eps, weight_decay;
    void* workspace; size_t workspace_bytes; void* stream;
    char* ws() const { return static_cast<char*>(workspace); }
    hipStream_t st() const { return static_cast<hipStream_t>(stream); }
};

// Adam arguments of step i of the call at learning rate lr (torch.optim.Adam's bias corrections); bc1 = 1 - beta1^t is what a
// member launch divides each member's own lr by (MemberLr)
struct AdamStep { AdamArgs adam; double bc1; };
inline AdamStep adam_step(const TrainCall& c, int64_t i, double lr) {
    const int64_t step = c.first_step + i;
    const double bc1 = 1.0 - pow(c.beta1, (double)step), bc2 = 1.0 - pow(c.beta2, (double)step);
    return AdamStep{AdamArgs{c.params, c.exp_avg, c.exp_avg_sq, lr / bc1, 1.0 / sqrt(bc2), c.beta1, c.beta2, c.eps,
                             c.weight_decay}, bc1};
}

// A schedule's row_begin[0 .. n] must be non-negative and strictly increasing: its largest batch, or -1
inline int64_t schedule_max_batch(int64_t n, const int64_t* row_begin) {
    int64_t bmax = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (row_begin[i + 1] <= row_begin[i] || row_begin[i] < 0) return -1;
        bmax = row_begin[i + 1] - row_begin[i] > bmax ? row_begin[i + 1] - row_begin[i] : bmax;
    }
    return bmax;
}

// What every schedule call is checked for once its model is known (P parameters, descriptor d): a gradient row holds the P
// gradients, sse and sum y^2; a QuanONet has its trunk input; the optimizer state is there; the schedule is well-formed.
// The largest batch, or -1 (QHEA_EINVAL).  n_steps and row_begin have been checked.
inline int64_t call_max_batch(const TrainCall& c, int64_t P, const qhea_model_desc& d) {
    if (c.grad_stride < P + 2) return -1;
    if (d.model == QHEA_MODEL_QUANONET && !c.trunk) return -1;
    if (!c.params || !c.exp_avg || !c.exp_avg_sq) return -1;
    return schedule_max_batch(c.n_steps, c.row_begin);
}

// Step i of the call: its rows and where its inputs and its gradient row begin (trunk: QuanONet only)
struct StepView {
    int64_t r0, nb;
    const double* branch; const double* trunk; const double* y;
    double* grad;
    double inv_bt;
};
inline StepView step_view(const TrainCall& c, int64_t i, const qhea_model_desc& d) {
    const int64_t r0 = c.row_begin[i];
    return StepView{r0, c.row_begin[i + 1] - r0, c.branch + r0 * d.branch_in,
                    d.model == QHEA_MODEL_QUANONET ? c.trunk + r0 * d.trunk_in : nullptr, c.y + r0,
                    c.grad + i * c.grad_stride, c.inv_batch_total[i]};
}

inline bool pauli_ok(int pauli, const double* ham_diag) {       // a diagonal Hamiltonian is a Z-basis object
    return pauli == QHEA_PAULI_Z || ((pauli == QHEA_PAULI_X || pauli == QHEA_PAULI_Y) && !ham_diag);
}

// the sweeps' member records: a known read-out (Z with ham_diag: every member reads out Z), nothing reserved, a finite lr >= 0
// (torch.optim.Adam refuses lr < 0 too)
inline bool member_records_ok(const qhea_member_hparams* members, int64_t n_models, const double* ham_diag) {
    for (int64_t m = 0; m < n_models; ++m) {
        const qhea_member_hparams& h = members[m];
        if (h.ham_pauli < QHEA_PAULI_Z || h.ham_pauli > QHEA_PAULI_Y || h.reserved != 0) return false;
        if (!pauli_ok(h.ham_pauli, ham_diag)) return false;
        if (!(h.lr >= 0.0) || !std::isfinite(h.lr)) return false;
    }
    return true;
}

}  // namespace qhea
