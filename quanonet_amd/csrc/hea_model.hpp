// hea_model.hpp -- the host's description of a circuit and of a model, for every translation unit: the run-length-encoded
// block list (Shape), a model descriptor resolved into it (ModelInfo), the table regions every workspace opens with and the
// model-level prep launch that fills them.  Declarations only: the definitions are in hea_api.hip.
#pragma once
#include <cstddef>
#include <cstdint>

#include "hea_device.hpp"

namespace qhea {

constexpr size_t kHeaderBytes = 256;        // WorkspaceHeader (hea_api.hip): the first bytes of every workspace
constexpr size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }           // every workspace region starts on 256 bytes
static_assert(align256(kHeaderBytes) == kHeaderBytes && kHeaderBytes == 256, "the header is one aligned unit of the layouts");

struct Shape {
    long E = 0, blk = 0;
    Runs runs{};
    int nblocks = 0;        // circuit blocks (the runs' counts added up)
    int fast_ld = 0;        // zyz_fast_ld: sub-layers per block of a block-unrolled shape (hea_zyz.hpp), 0: not one
};

// `count` more blocks of (enc, ld): they join the last run where it has the same (enc, ld), and open a run otherwise
int append_blocks(Shape& sh, long count, int enc, int ld);
// what closes a block list of nb blocks: the totals' range, nblocks, fast_ld
int finish_shape(int n, long nb, Shape& sh);
int make_shape(int n, int nb, const int32_t* enc, const int32_t* ld, Shape& sh);

// A model descriptor resolved.  Block list: nb[0] blocks of ld[0] sub-layers, then nb[1] blocks of ld[1] (QuanONet: trunk
// blocks, then branch blocks; HEAQNN: nb[1] = 0); every block opens with n encoding RX gates.  Encoding segment s (0: the first
// enc_cols[0] columns of x -- QuanONet: trunk, HEAQNN: the input --, 1: QuanONet's branch columns): x[b, e] =
// in[b, e % width] * w[e] + b[e] with trainable frequencies (off_w / off_b >= 0), in[b, e % width] * scale_coeff otherwise.
// off_*: indices in the flat parameter vector of P entries (-1: the model has none).
struct ModelInfo {
    Shape sh;
    int n = 0;
    int nb[2] = {0, 0}, ld[2] = {0, 0};
    long enc_cols[2] = {0, 0};
    int width[2] = {0, 0};
    bool trainable = false, has_bias = false;
    long P = 0, off_ans = 0, off_bias = -1, off_w[2] = {-1, -1}, off_b[2] = {-1, -1};
};

// QHEA_OK or what the descriptor is refused for
int model_info(const qhea_model_desc* d, ModelInfo& mi);

EncDesc make_enc(const qhea_model_desc* d, const ModelInfo& mi, const double* branch, const double* trunk, const double* params);

// prep_model_kernel for B rows: gate table entry g = s*n + q at gates[2 (g + n)] / gates[2 (g + n) + 1] (the two lane variants,
// n identity entries of padding on each side; (blk + 2) n pairs of double4 in all), cs[b * E + e] = (cos, sin)(x[b, e] / 2);
// hdr: the workspace header, which the kernel stamps
int launch_prep_model(const qhea_model_desc* d, const ModelInfo& mi, int64_t B, const double* branch, const double* trunk,
                      const double* params, double4* gates, double2* cs, void* hdr, hipStream_t st);

// What a workspace opens with: header, gate table, (cos, sin) table of B rows; `end` is where the caller's own regions begin
struct TableLayout { size_t off_gates, off_cs, end; };
inline TableLayout table_layout(int n, const Shape& sh, int64_t B) {
    TableLayout t{};
    t.off_gates = kHeaderBytes;
    t.off_cs = align256(t.off_gates + (size_t)(sh.blk + 2) * n * kGateBytes);
    t.end = align256(t.off_cs + (size_t)B * sh.E * sizeof(double2));
    return t;
}
inline TableLayout table_layout(const ModelInfo& mi, int64_t B) { return table_layout(mi.n, mi.sh, B); }

}  // namespace qhea
