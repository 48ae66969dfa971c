// hea_density.hip -- qhea_model_forward_noisy_exact: the model forward under the noise model of qhea_model_forward_noisy
// (include/quanonet_hea.h), computed exactly by carrying the density matrix rho through the circuit: per row the expectation of
// a read value and the standard deviation of one shot.  tests/density_reference.py restates it in numpy.
//
// Layout: vec(rho) of n qubits is a state of 2n index bits; bit 2q is wire q's row bit, bit 2q + 1 its column bit, so a gate on
// wire q touches two adjacent index bits and a CNOT with its channel four.  A row's 4^n elements live in LDS (16 bytes each); a
// thread owns 16 of them per pass: the elements that differ in the row and column bits of two wires.  4^(n-2) threads serve a
// row, a workgroup of 256 threads holds 256 / 4^(n-2) rows (256, 64, 16, 4, 1 for n = 2..6): always 64 KiB of state.
// A sub-layer is n passes; pass j loads wires (t, c) = (j, j + 1 mod n), applies the one-qubit gates still pending on them
// (the fused RY RZ RY, preceded by the encoding RX in a block's first sub-layer; wires 0 and 1 in pass 0, wire j + 1 in passes
// 1..n-2, none in the last) each with its depolarizing channel, then CNOT(c -> t) as a renaming of the 16 registers and the
// two-qubit channel, and stores.  One barrier per pass.  The low four bits of an element's LDS slot are XORed with the higher
// nibbles of its index (and with the row slot where several rows share a lane group), which spreads every pass' reads over the
// 16-byte bank quads.
//
// Read-out: H (X) or H S^dagger (Y) on every wire as one-qubit passes without noise; p = diag rho.  The readout confusion is
// symmetric, so it is applied to the value table instead of p: a workgroup mixes h[k] and h[k]^2 over the n bits once, before
// the circuit, and one thread per row adds p_k h'[k] and p_k h2'[k] in index order.  Nothing depends on the batch, the grid or
// other rows, and there are no atomics: a row's result is bitwise the same in any call.
#include "hea_density.hpp"

namespace qhea {
namespace {

template <int N>
__global__ __launch_bounds__(kDensThreads) void density_fwd_kernel(DensArgs a) {
    constexpr int TPR = 1 << (2 * N - 4), RPW = kDensThreads / TPR, D = 1 << N, NE = 1 << (2 * N);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];      // state, then h'[D], h2'[D]
    double2* state = reinterpret_cast<double2*>(dens_lds);
    double* hv = reinterpret_cast<double*>(dens_lds + kDensStateBytes);
    const int tid = threadIdx.x, slot = tid / TPR, rank = tid % TPR;
    long r = (long)blockIdx.x * RPW + slot;
    const bool live = r < a.B;
    if (!live) r = a.B - 1;                                              // a tail slot repeats the last row and stores nothing
    const double2* csr = a.cs + r * a.E;
    double2* row = state + slot * NE;
    const int sf = slot_fold<N>(slot);

    // value tables under the readout confusion: n two-point mixes of h and h^2
    double h = 0.0, h2 = 0.0;
    if (tid < D) {
        h = a.diag ? a.diag[tid] : a.off + a.co * (double)(N - 2 * (int)__popc(tid));
        h2 = h * h;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (tid < D) { hv[tid] = h; hv[D + tid] = h2; }
        __syncthreads();
        if (tid < D) {
            h = (1.0 - a.q) * h + a.q * hv[tid ^ (1 << i)];
            h2 = (1.0 - a.q) * h2 + a.q * hv[D + (tid ^ (1 << i))];
        }
        __syncthreads();
    }
    if (tid < D) { hv[tid] = h; hv[D + tid] = h2; }

    int s = 0, col = 0;
    bool first = true;
    for (int g = 0; g < 2; ++g) {
        for (int b = 0; b < a.nb[g]; ++b) {
            if (a.ld[g] == 0) {
                wire_passes<N, 0, 0>(row, rank, sf, a, csr, col, first);
                first = false;
            }
            for (int l = 0; l < a.ld[g]; ++l, ++s) {
                ring_passes<N, 0>(row, rank, sf, a, csr, s, col, l == 0, first);
                first = false;
            }
            col += N;
        }
    }
    if (first) {                                                         // no block at all: rho = |0><0|
        for (int i = rank; i < NE; i += TPR) row[i] = make_double2(0.0, 0.0);
        __syncthreads();
        if (rank == 0) row[fold(0) ^ sf] = make_double2(1.0, 0.0);
        __syncthreads();
    }
    if (a.pauli == QHEA_PAULI_X) wire_passes<N, 0, 1>(row, rank, sf, a, csr, 0, false);
    else if (a.pauli == QHEA_PAULI_Y) wire_passes<N, 0, 2>(row, rank, sf, a, csr, 0, false);

    if (rank == 0 && live) {
        double m1 = 0.0, m2 = 0.0;
        for (int k = 0; k < D; ++k) {
            int i = 0;
#pragma unroll
            for (int w = 0; w < N; ++w) i |= ((k >> w) & 1) * (3 << (2 * w));
            const double p = row[i ^ fold(i) ^ sf].x;
            m1 += p * hv[k];
            m2 += p * hv[D + k];
        }
        a.pred[r] = m1 + (a.bias ? a.bias[0] : 0.0);
        if (a.sd) {
            const double var = m2 - m1 * m1;
            a.sd[r] = var > 0.0 ? sqrt(var) : 0.0;
        }
    }
}

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_exact_noisy_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (batch < 0 || model_info(desc, mi) != QHEA_OK) return 0;
    return dens_layout(mi, batch).total;
}

int qhea_model_forward_noisy_exact(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                                   const double* params, const double* ham_diag, const qhea_noise* noise, double* pred,
                                   double* shot_std, void* workspace, size_t workspace_bytes, void* stream) {
    NoisyCall c;
    int rc = noisy_call_check({QHEA_MIN_QUBITS, 6 /* 4^n elements per row in LDS */, false, false}, desc, ham_diag, noise, 0,
                              batch, trunk, {branch, params, pred}, workspace, stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    const DensLayout L = dens_layout(c.mi, batch);
    if (!workspace || workspace_bytes < L.total) return QHEA_EWORKSPACE;
    double4* gates = reinterpret_cast<double4*>(c.ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(c.ws + L.off_cs);
    rc = launch_prep_model(desc, c.mi, batch, branch, trunk, params, gates, cs, c.ws, c.st);
    if (rc != QHEA_OK) return rc;

    DensArgs a = dens_args(desc, c.mi, noise, params, ham_diag, batch, gates, cs);
    a.pred = pred; a.sd = shot_std;
    return dispatch_n(c.mi.n, [&](auto n) { return launch_density_fwd<n()>(density_fwd_kernel<n()>, a, c.st); });
}

}  // extern "C"
