// hea_noise.hpp -- what hea_noise.hip (the noisy forward, qhea_model_forward_noisy) takes from hea_api.hip: a model's block
// list and the model-level prep kernel that fills the gate table and the per-row (cos, sin) table.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/quanonet_hea.h"

namespace qhea {

// Block list of a model descriptor: nb[0] blocks of ld[0] sub-layers, then nb[1] blocks of ld[1] (QuanONet: trunk blocks, then
// branch blocks; HEAQNN: nb[1] = 0).  Every block opens with n encoding RX gates.  blk = total sub-layers, E = encoding columns,
// off_bias = the model bias' index in the flat parameter vector (-1: no bias).
struct NoiseShape {
    int n, blk, E;
    int nb[2], ld[2];
    long off_bias;
};

// QHEA_OK or the descriptor's error (model_info's checks)
int noise_model_shape(const qhea_model_desc* d, NoiseShape& ns);

// prep_model_kernel for B rows: gate table entry g = s*n + q at gates[2 (g + n)] / gates[2 (g + n) + 1] (the two lane variants,
// n identity entries of padding on each side; (blk + 2) n pairs of double4 in all), cs[b * E + e] = (cos, sin)(x[b, e] / 2);
// hdr: a 256-byte workspace header the kernel stamps
int launch_noise_prep(const qhea_model_desc* d, int64_t B, const double* branch, const double* trunk, const double* params,
                      double4* gates, double2* cs, void* hdr, hipStream_t st);

// Where a model's gradients live in the flat parameter vector, and what feeds each encoding segment (segment 0: the first
// ncols[0] columns of x -- QuanONet: trunk, HEAQNN: the input --, segment 1: QuanONet's branch columns): x[b, e] =
// in[b, e % width] * w[e] + b[e] with trainable frequencies (off_w / off_b >= 0), in[b, e % width] * scale_coeff otherwise.
struct NoiseGradMap {
    long P, off_ans;
    long off_w[2], off_b[2];
    int ncols[2], width[2];
};
int noise_model_grad_map(const qhea_model_desc* d, NoiseGradMap& gm);

}  // namespace qhea
