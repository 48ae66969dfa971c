// hea_qsweep.hpp -- qubit sweeps (qhea_model_qubit_sweep_train_steps): members of different qubit counts trained side by side.
// The wave-resident members with n = 2..6 are split into register classes -- runs of consecutive n whose packed backward
// kernels give the same waves per SIMD -- and each class is one backward launch per step, whose workgroups take
// their (member, sample group) from a host-built work list.  n = 7..9 take one launch per n (QubitArgs), and so do the
// workgroup-resident members, n = 10..12 (lds_bwd_kernel<N, QubitArgs>, hea_lds.hip: DESIGN.md 7e).
#pragma once
#include "hea_device.hpp"
#include "hea_zyz.hpp"

namespace qhea {

// Register classes of the packed backward kernel (bwd_kernel<N, 1, DepthArgs>, -Rpass-analysis=kernel-resource-usage):
// n = 2 134 VGPRs (3 waves per SIMD); n = 3..6 182..240 VGPRs (2).  n = 7..9 (230 VGPRs / 256 + AGPRs) run the member form of
// bwd_kernel itself, one launch per n (QubitArgs): a copy of its body inlined into a class kernel rounds differently there
// (DESIGN.md 7d).
constexpr int kQsClasses = 2;
constexpr int kQsOwnLo = 7, kQsOwnHi = 9;       // n with a launch of their own
__host__ __device__ constexpr int qs_class_lo(int c) { return c == 0 ? 2 : 3; }
__host__ __device__ constexpr int qs_class_hi(int c) { return c == 0 ? 2 : 6; }
__host__ __device__ constexpr int qs_class_of(int n) { return n <= 2 ? 0 : n <= 6 ? 1 : -1; }
// is the wave-resident kernel of n part of this build (QHEA_SUBSET)?
#define QHEA_QS_OR(NN) || n == NN
__host__ __device__ constexpr bool qs_built(int n) { return false QHEA_FOR_EACH_N(QHEA_QS_OR); }
#undef QHEA_QS_OR

// the packed backward kernel's waves (a multiple of kWaves) for B samples of n qubits -- its partial rows
__host__ __device__ inline long qs_nwaves(int n, long B) {
    const int spw = 64 >> lane_bits(n);
    return (((B + spw - 1) / spw + kWaves - 1) / kWaves) * kWaves;
}

// a member's partial rows: the packed backward kernel's waves (n <= 9), one row per sample for the workgroup-resident kernel
// (n >= 10, hea_lds.hip)
__host__ __device__ inline long qs_part_rows(int n, long B) { return n >= 10 ? B : qs_nwaves(n, B); }

// Work lists: entries (member, sample group) of the backward launches -- (member, 0) for the launches of one n, 7..12 -- and
// (member, role) of the reduce launch, 8 bytes each,
// in the list regions of the members' workspace slices -- entry k is entry k % per of slice k / per's region, which starts at
// `list` + (k / per) * slice bytes.  Written once per call (work_fill_kernel, hea_api.hip), read with one scalar load per
// workgroup.  base: the launch's first entry.
struct QsWork {
    const char* list;           // slice 0's list region
    int per;                    // entries per slice
    int base;
};
typedef const __attribute__((address_space(4))) int* ConstQsEntry;
__device__ __forceinline__ int2 qs_entry(const QsWork& w, long slice_bytes, int i) {
    const int k = w.base + i;
    const ConstQsEntry e = (ConstQsEntry)(w.list + (long)(k / w.per) * slice_bytes + (long)(k % w.per) * (long)sizeof(int2));
    return make_int2(e[0], e[1]);
}

// Arguments of a class's backward launch.  Pointers are member 0's (slice 0, row 0); member m's move as in DepthArgs.
// runs[n - 2]: the run table of n -- two runs (enc = n, ld = the shared linear depths) whose counts are each member's
// MemberRec::depth.
struct QubitBwdArgs {
    Runs runs[8];
    long B;
    double inv_bt;
    const double2* cs;
    const char* gates;
    const double* y;
    const double* bias;         // QuanONet: member 0's parameter row (the bias is its first entry); HEAQNN: nullptr
    double* out;
    double* grad_x;
    double* partial;
    const char* mrec;           // member 0's MemberRec
    MemberStride ms;
    QsWork wk;
};

void launch_bwd_qsweep_0(dim3 grid, hipStream_t st, const QubitBwdArgs& a);
void launch_bwd_qsweep_1(dim3 grid, hipStream_t st, const QubitBwdArgs& a);

// n = 7..9: bwd_kernel<N, MINW, QubitArgs> (hea_inst.hip), member = entry blockIdx.y of the list (the members of that n),
// sample group = blockIdx.x; otherwise the prologue of DepthArgs
struct QubitArgs {
    const char* mrec;           // member 0's MemberRec
    MemberStride ms;
    QsWork wk;
    __device__ __forceinline__ long member() const { return qs_entry(wk, ms.ws, (int)blockIdx.y).x; }
    __device__ __forceinline__ ConstMemberRec rec() const {
        return (ConstMemberRec)member_ptr(reinterpret_cast<const MemberRec*>(mrec), ws_bytes());
    }
    __device__ __forceinline__ long ws_bytes() const { return member() * ms.ws; }
    __device__ __forceinline__ long row_bytes() const { return member() * ms.rows * (long)sizeof(double); }
    __device__ __forceinline__ long param_bytes() const { return member() * ms.params * (long)sizeof(double); }
};
#define QHEA_QDECLARE(NN) void launch_bwd_qubit_##NN(dim3 grid, hipStream_t st, const BwdArgs& a, const QubitArgs& q);
QHEA_FOR_EACH_N(QHEA_QDECLARE)
#undef QHEA_QDECLARE

// n = 10..12 (hea_lds.hip): the member forms of the workgroup-resident backward kernel, lds_bwd_kernel<N, DepthArgs> (member =
// blockIdx.y: depth sweeps, ensembles and sweeps) and lds_bwd_kernel<N, QubitArgs> (member = work-list entry blockIdx.y: qubit
// sweeps); grid.x = the batch, one workgroup per sample as in the single-model launch.  a: as for launch_lds_bwd, member 0's
// pointers, its E / blk / read-out unused (the member's come from its MemberRec); QHEA_EUNSUPPORTED for other n.
int launch_lds_bwd_depth(int n, dim3 grid, hipStream_t st, const BwdArgs& a, const DepthArgs& d);
int launch_lds_bwd_qubit(int n, dim3 grid, hipStream_t st, const BwdArgs& a, const QubitArgs& q);

}  // namespace qhea
