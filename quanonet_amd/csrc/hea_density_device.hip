// hea_density_device.hip -- qhea_model_forward_noisy_device_exact and qhea_device_noise_tables: the exact noisy forward of
// hea_density.hip under the calibrated device noise model of include/quanonet_hea.h (qhea_device_noise): per-wire one-qubit
// and per-slot CNOT depolarizing rates, T1 / T2 relaxation over the timeline of a sub-layer (the idle decay of the sequential
// CNOT ring included) and an asymmetric readout error per bit.  tests/device_noise_reference.py restates the model in numpy,
// channel by channel and slot by slot.
//
// Every one-wire channel of the model is phase-covariant: a triple (off, a, b) that scales the wire's off-diagonal elements
// by `off` and maps z = rho00 - rho11 to a z + b tr.  Relaxation of one wire commutes with everything on the other wires, so
// the host composes all of a wire's channels between two of its gates into one triple: four sites per wire (after the
// encoding RX, after the fused rotation, after the slot where the wire is control, after the slot where it is target).  The
// kernel is density_fwd_kernel with those triples in place of the uniform channels: layout, passes, barriers, grid and the
// determinism rules are hea_density.hip's.  The tables are members of the by-value argument record, in the form the kernel
// multiplies with, and are indexed by compile-time constants only (the pass' wires, the site): each entry is a scalar of the
// launch, read with scalar loads, and no table is indexed by a run-time value.  There are 24 n doubles of them (144 at
// n = 6, two scalar registers each), more than a wave's scalar registers hold: the compiler loads them all at entry and keeps
// the overflow in lanes of 1-4 vector registers (v_writelane / v_readlane, no memory; profiles/r19_resource_usage.txt).
#include "hea_density.hpp"
#include "hea_device_noise.hpp"

namespace qhea {
namespace {

struct DensDevArgs {
    const double4* gates;                   // prep table, entry 0 = padding entry -n
    const double2* cs;                      // [B, E]
    const double* diag;                     // ham_diag or NULL
    const double* bias;                     // model bias or NULL
    double off, co;                         // H = off + co sum P_i
    double chan[4][kDevMaxWires][5];        // [site][wire] (off, k00, k01, k10, k11): the triple's element form
    double keep2[kDevMaxWires], mix2[kDevMaxWires];     // two-qubit channel of slot j: 1 - lam, lam / 4 (lam = 16 p2[j] / 15)
    double r01[kDevMaxWires], r10[kDevMaxWires];    // P(read 1 | 0), P(read 0 | 1) per bit
    long B;
    int E, pauli;
    int nb[2], ld[2];
    double* pred;
    double* sd;                             // or NULL
};

// the phase-covariant channel (off, a, b) of site SITE, wire Q on the 2 x 2 blocks of that wire (phase_covariant of
// hea_density.hpp), its constants scalars of the launch
template <int S, int SITE, int Q>
__device__ __forceinline__ void channel1(double2 (&e)[16], const DensDevArgs& a) {
    phase_covariant<S>(e, a.chan[SITE][Q][0], a.chan[SITE][Q][1], a.chan[SITE][Q][2], a.chan[SITE][Q][3], a.chan[SITE][Q][4]);
}

// wire Q's pending gates of sub-layer s: (encoding RX, its site), fused RY RZ RY, its site
template <int N, int S, int Q>
__device__ __forceinline__ void dev_wire_gates(double2 (&e)[16], const DensDevArgs& a, const double2* csr, int s, int col,
                                               bool enc) {
    if (enc) {
        const double2 c = csr[col + Q];
        apply_gate<S>(e, encoding_rx(c));
        channel1<S, kEnc, Q>(e, a);
    }
    const double4 v = a.gates[2 * (s * N + Q + N)];                      // (u00, u01); u10 = -conj(u01), u11 = conj(u00)
    apply_gate<S>(e, U2{{v.x, v.y}, {v.z, v.w}, {-v.z, v.w}, {v.x, -v.y}});
    channel1<S, kRot, Q>(e, a);
}

// ring_passes of hea_density.hpp with the device channels: slot J's CNOT, its two-qubit channel, then the target site of
// wire J and the control site of wire J + 1 mod N
template <int N, int J>
__device__ __forceinline__ void dev_ring_passes(double2* row, int rank, int sf, const DensDevArgs& a, const double2* csr, int s,
                                                int col, bool enc, bool first) {
    if constexpr (J < N) {
        using P = Pass<N, J>;
        const int i0 = P::base(rank), b = i0 ^ fold(i0) ^ sf;
        double2 e[16];
        if (J == 0 && first) {                                           // rho = |0><0|
#pragma unroll
            for (int k = 0; k < 16; ++k) e[k] = make_double2(k == 0 && rank == 0 ? 1.0 : 0.0, 0.0);
        } else {
            P::load(e, row, b);
        }
        if (J == 0) dev_wire_gates<N, 1, P::t>(e, a, csr, s, col, enc);
        if (J <= N - 2) dev_wire_gates<N, 4, P::c>(e, a, csr, s, col, enc);
        cnot_depolarize2(e, a.keep2[J], a.mix2[J]);
        channel1<1, kTgt, P::t>(e, a);
        channel1<4, kCtl, P::c>(e, a);
        P::store(e, row, b);
        __syncthreads();
        dev_ring_passes<N, J + 1>(row, rank, sf, a, csr, s, col, enc, false);
    }
}

// a block without sub-layers: the encoding RX of every wire with its site, two wires per pass (wire_passes, KIND 0)
template <int N, int J>
__device__ __forceinline__ void dev_enc_passes(double2* row, int rank, int sf, const DensDevArgs& a, const double2* csr, int col,
                                               bool first) {
    if constexpr (J < N) {
        using P = Pass<N, J>;
        const int i0 = P::base(rank), b = i0 ^ fold(i0) ^ sf;
        double2 e[16];
        if (J == 0 && first) {
#pragma unroll
            for (int k = 0; k < 16; ++k) e[k] = make_double2(k == 0 && rank == 0 ? 1.0 : 0.0, 0.0);
        } else {
            P::load(e, row, b);
        }
        const double2 c0 = csr[col + P::t];
        apply_gate<1>(e, encoding_rx(c0));
        channel1<1, kEnc, P::t>(e, a);
        if (J + 1 < N) {
            const double2 c1 = csr[col + P::c];
            apply_gate<4>(e, encoding_rx(c1));
            channel1<4, kEnc, P::c>(e, a);
        }
        P::store(e, row, b);
        __syncthreads();
        dev_enc_passes<N, J + 2>(row, rank, sf, a, csr, col, false);
    }
}

template <int N>
__global__ __launch_bounds__(kDensThreads) void density_dev_fwd_kernel(DensDevArgs a) {
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

    // value tables under the readout confusion: per bit, h'[k] = (1 - f) h[k] + f h[k ^ bit], f = P(the bit of k is misread)
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
            const double f = (tid >> i) & 1 ? a.r10[i] : a.r01[i];
            h = (1.0 - f) * h + f * hv[tid ^ (1 << i)];
            h2 = (1.0 - f) * h2 + f * hv[D + (tid ^ (1 << i))];
        }
        __syncthreads();
    }
    if (tid < D) { hv[tid] = h; hv[D + tid] = h2; }                      // read after the barriers of the passes below

    int s = 0, col = 0;
    bool first = true;
    for (int g = 0; g < 2; ++g) {
        for (int b = 0; b < a.nb[g]; ++b) {
            if (a.ld[g] == 0) {
                dev_enc_passes<N, 0>(row, rank, sf, a, csr, col, first);
                first = false;
            }
            for (int l = 0; l < a.ld[g]; ++l, ++s) {
                dev_ring_passes<N, 0>(row, rank, sf, a, csr, s, col, l == 0, first);
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
    const DensArgs none{};                                               // the basis-change passes read nothing of it
    if (a.pauli == QHEA_PAULI_X) wire_passes<N, 0, 1>(row, rank, sf, none, csr, 0, false);
    else if (a.pauli == QHEA_PAULI_Y) wire_passes<N, 0, 2>(row, rank, sf, none, csr, 0, false);

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

int qhea_device_noise_tables(int n, const qhea_device_noise* dn, double* chan, double* lam2) {
    const int rc = device_noise_check(n, dn);
    if (rc != QHEA_OK) return rc;
    if (!chan || !lam2) return QHEA_EINVAL;
    device_noise_compose(n, dn, chan, n, lam2);
    return QHEA_OK;
}

int qhea_model_forward_noisy_device_exact(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                                          const double* params, const double* ham_diag, const qhea_device_noise* dn,
                                          double* pred, double* shot_std, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    NoisyCall c;
    int rc = device_call_check({QHEA_MIN_QUBITS, kDevMaxWires /* 4^n elements per row in LDS */, false, false}, desc, ham_diag, dn,
                               nullptr, batch, trunk, {branch, params, pred}, workspace, stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    const DensLayout L = dens_layout(c.mi, batch);
    if (!workspace || workspace_bytes < L.total) return QHEA_EWORKSPACE;
    double4* gates = reinterpret_cast<double4*>(c.ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(c.ws + L.off_cs);
    rc = launch_prep_model(desc, c.mi, batch, branch, trunk, params, gates, cs, c.ws, c.st);
    if (rc != QHEA_OK) return rc;

    const int n = c.mi.n;
    DensDevArgs a{};
    circuit_args(a, desc, c.mi, params, ham_diag, batch, gates, cs);
    const DevSites sites(n, dn);
    for (int q = 0; q < n; ++q) {
        for (int k = 0; k < 4; ++k) element_form(sites.at(k, q), a.chan[k][q]);
        slot_form(sites.lam2[q], a.keep2[q], a.mix2[q]);
        a.r01[q] = dn->readout01[q]; a.r10[q] = dn->readout10[q];
    }
    a.pred = pred; a.sd = shot_std;
    return dispatch_n(n, [&](auto nn) { return launch_density_fwd<nn()>(density_dev_fwd_kernel<nn()>, a, c.st); });
}

}  // extern "C"
