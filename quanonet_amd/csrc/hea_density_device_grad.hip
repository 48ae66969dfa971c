// hea_density_device_grad.hip -- qhea_model_loss_grad_noisy_device_exact / qhea_model_train_steps_noisy_device_exact: the MSE
// loss of the exact noisy forward under the calibrated device noise model (hea_density_device.hip) and its exact gradient.  The
// contract is stated in include/quanonet_hea.h; tests/device_noise_grad_reference.py restates the walk in numpy with Kraus
// operators.
//
// density_dev_bwd_kernel<N> is density_bwd_kernel<N> (hea_density_grad.hip) with the channel sites of the device model: layout,
// fold, passes, barriers, rows per workgroup, LDS budget, trace sums and the record are that kernel's (hea_density_grad.hpp).
// What differs is the channel algebra.  A one-wire site is a phase-covariant triple (off, a, b), and it is not self-adjoint
// once b != 0, so the reverse walk needs three forms of every site:
//   forward (the sweep that carries rho to the end)   rho00' = k00 rho00 + k01 rho11, rho11' = k10 rho00 + k11 rho11, off;
//   inverse (rho walks back)                          the same with the triple (1 / off, 1 / a, -b / a);
//   adjoint (O walks back)                            O00' = k00 O00 + k10 O11, O11' = k01 O00 + k11 O11, off.
// In slot J the forward applies CNOT, D2(lam_J), TGT of wire J, CTL of wire J + 1 mod n; the reverse pass undoes the two sites
// first, then D2 (self-adjoint; its inverse is hea_density_grad's with the slot's own lam), then the CNOT.  A wire's pending
// gates are followed by their ENC / ROT site: in reverse the site's inverse on rho and adjoint on O, then the trace, then the
// un-rotation.
//
// Constants.  3 forms x 4 sites x 5 doubles per wire, the slot's four D2 factors and the wire's two readout probabilities are 66
// doubles per wire, 396 at n = 6: by-value arguments indexed by compile-time constants, as the forward kernel holds its 24 n,
// would be parked in vector registers the walk has none left of.  dev_table_kernel (one workgroup, launched once per call)
// copies them from its by-value argument into the workspace; the backward kernel reads a site's constants where it uses them,
// from an address it forms behind a scalar zero the compiler cannot see through (so the loads stay inside their pass), and
// moves them to scalar registers (the address is wave-uniform).
//
// Stored states.  The inverse walk amplifies the traceless part of rho by A_dev, so the calls above refuse log10 A_dev > 7.
// qhea_model_loss_grad_noisy_device_exact_stored / ..._train_steps_..._stored run density_dev_stored_bwd_kernel<N>: the same
// kernel, except that its forward sweep writes rho after every unit -- a sub-layer, or the encoding gates of a block without
// sub-layers -- to the workspace and its reverse walk starts every unit from the stored state (fetched into registers one
// unit ahead, so that the loads land while the unit in front is walked).  Within a unit nothing differs, so the guard is
// asked of one unit only.
// The record layout of the table, the scalar reads, a site in reverse and the guard's log10 A_dev sit in
// hea_density_device_grad.hpp, which hea_density_device_wide_grad.hip (n = 7..9 on tiles) shares.
#include "hea_density_device_grad.hpp"

namespace qhea {
namespace {

struct DevTable { double v[kTabDoubles]; };

__global__ __launch_bounds__(64) void dev_table_kernel(DevTable t, double* out) {
    for (int i = threadIdx.x; i < kTabDoubles; i += 64) out[i] = t.v[i];
}

struct DevGradArgs {
    const double4* gates;                   // prep table, entry 0 = padding entry -n
    const double2* cs;                      // [B, E]
    const double* diag;                     // ham_diag or NULL
    const double* bias;                     // model bias or NULL
    const double* tab;                      // [kTabDoubles], written by dev_table_kernel
    const double* w;                        // ansatz angles [blk, 3, n]
    double off, co;                         // H = off + co sum P_i
    long B;
    int E, pauli;
    int nb[2], ld[2];
    double* pred;                           // the caller's pred or NULL
    double* pred_ws;                        // [B]
    double* rec;                            // [E + 3 n blk][B]: d pred_b / d x[b, e], then d pred_b / d w[s, k, q]
};

// ... of the stored-state kernel: the record above and where the forward sweep leaves rho after every unit
struct DevStoredArgs : DevGradArgs {
    double2* snap;                          // [U][B][4^n]: snap[u][row] = the row's rho after unit u, as its image in LDS
};

// ---- forward sweep: the passes of density_dev_fwd_kernel with the constants read from the table ----
// dev_wire_gates, dev_ring_passes and dev_enc_passes below are hea_density_device.hip's functions of the same names, statement
// for statement (the channel bodies they call, phase_covariant and cnot_depolarize2 of hea_density.hpp, are shared); only where a
// site's constants come from differs (there: members of the by-value argument indexed at compile time; here: the workspace
// table, loaded inside the pass).  Templated over that source they changed this unit's code (profiles/
// r28_device_code_identity.txt), so a change to the forward model is made in both; tests/test_device_noise_training.py holds
// this sweep's pred to the forward call's within 1e-13.

template <int N, int S>
__device__ __forceinline__ void dev_wire_gates(double2 (&e)[16], const DevGradArgs& a, const double* tab, const double2* csr,
                                               int s, int col, bool enc, int q) {
    if (enc) {
        const double2 c = csr[col + q];
        apply_gate<S>(e, encoding_rx(c));
        channel5<S>(e, site_at(tab, q, kEnc, kFormFwd));
    }
    const double4 v = a.gates[2 * (s * N + q + N)];                      // (u00, u01); u10 = -conj(u01), u11 = conj(u00)
    apply_gate<S>(e, U2{{v.x, v.y}, {v.z, v.w}, {-v.z, v.w}, {v.x, -v.y}});
    channel5<S>(e, site_at(tab, q, kRot, kFormFwd));
}

template <int N, int J>
__device__ __forceinline__ void dev_ring_passes(double2* row, int rank, int sf, const DevGradArgs& a, const double2* csr, int s,
                                                int col, bool enc, bool first) {
    if constexpr (J < N) {
        using P = Pass<N, J>;
        const int i0 = P::base(rank), b = i0 ^ fold(i0) ^ sf;
        const double* tab = a.tab + opaque_szero();
        double2 e[16];
        if (J == 0 && first) {                                           // rho = |0><0|
#pragma unroll
            for (int k = 0; k < 16; ++k) e[k] = make_double2(k == 0 && rank == 0 ? 1.0 : 0.0, 0.0);
        } else {
            P::load(e, row, b);
        }
        if (J == 0) dev_wire_gates<N, 1>(e, a, tab, csr, s, col, enc, P::t);
        if (J <= N - 2) dev_wire_gates<N, 4>(e, a, tab, csr, s, col, enc, P::c);
        cnot_depolarize2(e, uniform_load(tab + J * kTabWire + kTabSlot), uniform_load(tab + J * kTabWire + kTabSlot + 1));
        channel5<1>(e, site_at(tab, P::t, kTgt, kFormFwd));
        channel5<4>(e, site_at(tab, P::c, kCtl, kFormFwd));
        P::store(e, row, b);
        __syncthreads();
        dev_ring_passes<N, J + 1>(row, rank, sf, a, csr, s, col, enc, false);
    }
}

template <int N, int J>
__device__ __forceinline__ void dev_enc_passes(double2* row, int rank, int sf, const DevGradArgs& a, const double2* csr, int col,
                                               bool first) {
    if constexpr (J < N) {
        using P = Pass<N, J>;
        const int i0 = P::base(rank), b = i0 ^ fold(i0) ^ sf;
        const double* tab = a.tab + opaque_szero();
        double2 e[16];
        if (J == 0 && first) {
#pragma unroll
            for (int k = 0; k < 16; ++k) e[k] = make_double2(k == 0 && rank == 0 ? 1.0 : 0.0, 0.0);
        } else {
            P::load(e, row, b);
        }
        const double2 c0 = csr[col + P::t];
        apply_gate<1>(e, encoding_rx(c0));
        channel5<1>(e, site_at(tab, P::t, kEnc, kFormFwd));
        if (J + 1 < N) {
            const double2 c1 = csr[col + P::c];
            apply_gate<4>(e, encoding_rx(c1));
            channel5<4>(e, site_at(tab, P::c, kEnc, kFormFwd));
        }
        P::store(e, row, b);
        __syncthreads();
        dev_enc_passes<N, J + 2>(row, rank, sf, a, csr, col, false);
    }
}

// ---- reverse walk ----
// wire q's gates of sub-layer s in reverse; tr[k] = this thread's share of d pred / d w[s, k, q], tr[3] of d pred / d x[col + q]
template <int N, int S>
__device__ __forceinline__ void dev_undo_wire(double2 (&e)[16], double2 (&o)[16], const DevGradArgs& a, const double* tab,
                                              const double2* csr, int s, int col, bool enc, int q, double* tr) {
    undo_site<S>(e, o, tab, q, kRot);
    undo_rotations<N, S>(e, o, a.w, s, q, tr);
    if (enc) dev_undo_encoding<S>(e, o, tab, q, csr[col + q], tr);
}

// the reverse of dev_ring_passes: passes J = N - 1 .. 0 of sub-layer s
template <int N, int J>
__device__ __forceinline__ void dev_ring_passes_back(RowCtx<N>& cx, const DevGradArgs& a, const double2* csr, int s, int col,
                                                     bool enc) {
    if constexpr (J >= 0) {
        using P = Pass<N, J>;
        const int i0 = P::base(cx.rank | opaque_zero()), b = i0 ^ fold(i0) ^ cx.sf;
        const double* tab = a.tab + opaque_szero();
        double2 e[16], o[16];
        P::load(e, cx.rho, b);
        P::load(o, cx.obs, b);
        undo_site<1>(e, o, tab, P::t, kTgt);
        undo_site<4>(e, o, tab, P::c, kCtl);
        const double* sl = tab + J * kTabWire + kTabSlot;
        undo_cnot2(e, uniform_load(sl + 2), uniform_load(sl + 3));
        undo_cnot2(o, uniform_load(sl), uniform_load(sl + 1));
        double tr[kTracesPerPass];
        int idx[kTracesPerPass];
#pragma unroll
        for (int i = 0; i < kTracesPerPass; ++i) { tr[i] = 0.0; idx[i] = -1; }
        const int ans = a.E + s * 3 * N;
        if (J <= N - 2) {
            dev_undo_wire<N, 4>(e, o, a, tab, csr, s, col, enc, P::c, tr);
            idx[0] = ans + P::c; idx[1] = ans + N + P::c; idx[2] = ans + 2 * N + P::c; idx[3] = enc ? col + P::c : -1;
        }
        if (J == 0) {
            dev_undo_wire<N, 1>(e, o, a, tab, csr, s, col, enc, P::t, tr + 4);
            idx[4] = ans + P::t; idx[5] = ans + N + P::t; idx[6] = ans + 2 * N + P::t; idx[7] = enc ? col + P::t : -1;
        }
        P::store(e, cx.rho, b);
        P::store(o, cx.obs, b);
        if (J <= N - 2) flush_traces<N>(cx, a, tr, idx);
        else __syncthreads();
        dev_ring_passes_back<N, J - 1>(cx, a, csr, s, col, enc);
    }
}

// the reverse of dev_enc_passes: a block without sub-layers, its encoding gates only
template <int N, int J>
__device__ __forceinline__ void dev_enc_passes_back(RowCtx<N>& cx, const DevGradArgs& a, const double2* csr, int col) {
    if constexpr (J < N) {
        using P = Pass<N, J>;
        const int i0 = P::base(cx.rank | opaque_zero()), b = i0 ^ fold(i0) ^ cx.sf;
        const double* tab = a.tab + opaque_szero();
        double2 e[16], o[16];
        P::load(e, cx.rho, b);
        P::load(o, cx.obs, b);
        double tr[kTracesPerPass];
        int idx[kTracesPerPass];
#pragma unroll
        for (int i = 0; i < kTracesPerPass; ++i) { tr[i] = 0.0; idx[i] = -1; }
        dev_undo_encoding<1>(e, o, tab, P::t, csr[col + P::t], tr);
        idx[3] = col + P::t;
        if (J + 1 < N) {
            dev_undo_encoding<4>(e, o, tab, P::c, csr[col + P::c], tr + 4);
            idx[7] = col + P::c;
        }
        P::store(e, cx.rho, b);
        P::store(o, cx.obs, b);
        flush_traces<N>(cx, a, tr, idx);
        dev_enc_passes_back<N, J + 2>(cx, a, csr, col);
    }
}

template <int N>
__global__ __launch_bounds__(bwd_threads<N>()) void density_dev_bwd_kernel(DevGradArgs a) {
    using C = RowCtx<N>;
    constexpr int TPR = C::TPR, RPW = bwd_threads<N>() / TPR, D = 1 << N, NE = 1 << (2 * N);
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];      // rho, O, h'[D], the waves' trace partials
    double2* state = reinterpret_cast<double2*>(dens_lds);
    double* hv = reinterpret_cast<double*>(dens_lds + 2 * RPW * NE * sizeof(double2));
    const int tid = threadIdx.x, slot = tid / TPR, rank = tid % TPR;
    long r = (long)blockIdx.x * RPW + slot;
    const bool live = r < a.B;
    if (!live) r = a.B - 1;                                              // a tail slot repeats the last row and stores nothing
    const double2* csr = a.cs + r * a.E;
    C cx;
    cx.rho = state + slot * NE;
    cx.obs = state + RPW * NE + slot * NE;
    cx.red = hv + D;
    cx.rank = rank; cx.sf = slot_fold<N>(slot); cx.parity = 0;
    cx.r = r; cx.B = a.B; cx.live = live;
    double2* row = cx.rho;
    const int sf = cx.sf;

    // value table under the readout confusion: per bit, h'[k] = (1 - f) h[k] + f h[k ^ bit], f = P(the bit of k is misread)
    double h = 0.0;
    if (tid < D) h = a.diag ? a.diag[tid] : a.off + a.co * (double)(N - 2 * (int)__popc(tid));
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (tid < D) hv[tid] = h;
        __syncthreads();
        if (tid < D) {
            const double f = a.tab[i * kTabWire + kTabRead + ((tid >> i) & 1)];
            h = (1.0 - f) * h + f * hv[tid ^ (1 << i)];
        }
        __syncthreads();
    }
    if (tid < D) hv[tid] = h;

    // forward sweep: the passes of density_dev_fwd_kernel
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
        double m1 = 0.0;
        for (int k = 0; k < D; ++k) {
            int i = 0;
#pragma unroll
            for (int w = 0; w < N; ++w) i |= ((k >> w) & 1) * (3 << (2 * w));
            m1 += row[i ^ fold(i) ^ sf].x * hv[k];
        }
        const double p = m1 + (a.bias ? a.bias[0] : 0.0);
        a.pred_ws[r] = p;
        if (a.pred) a.pred[r] = p;
    }

    // O = diag h' in the read-out basis
    for (int i = rank; i < NE; i += TPR) {
        int k = 0;
        bool diag = true;
#pragma unroll
        for (int w = 0; w < N; ++w) {
            const int rb = (i >> (2 * w)) & 1, cb = (i >> (2 * w + 1)) & 1;
            diag = diag && rb == cb;
            k |= rb << w;
        }
        cx.obs[i ^ fold(i) ^ sf] = make_double2(diag ? hv[k] : 0.0, 0.0);
    }
    __syncthreads();
    // back to the computational basis: rho and O through the daggers of the basis change
    if (a.pauli == QHEA_PAULI_X) {
        basis_passes_back<N, 0, 3>(cx.rho, rank, sf);
        basis_passes_back<N, 0, 3>(cx.obs, rank, sf);
    } else if (a.pauli == QHEA_PAULI_Y) {
        basis_passes_back<N, 0, 4>(cx.rho, rank, sf);
        basis_passes_back<N, 0, 4>(cx.obs, rank, sf);
    }

    // reverse walk: blocks, sub-layers and passes in reverse order
    for (int g = 1; g >= 0; --g) {
        for (int b = a.nb[g] - 1; b >= 0; --b) {
            col -= N;
            for (int l = a.ld[g] - 1; l >= 0; --l) {
                --s;
                dev_ring_passes_back<N, N - 1>(cx, a, csr, s, col, l == 0);
            }
            if (a.ld[g] == 0) dev_enc_passes_back<N, 0>(cx, a, csr, col);
        }
    }
}

// ---- stored states ----
// A unit is one sub-layer (a block's first carries its encoding) or the encoding gates of a block without sub-layers.  The row's
// image in LDS is copied as it lies (fold and slot fold included: the thread that stored an element is the one that loads it),
// element i by the row's thread i mod TPR: 16 bytes per lane, contiguous over the row's lanes.  A tail slot copies nothing.
// Called by every thread of the workgroup behind a pass' closing barrier; the barrier inside closes the copy.
template <int N>
__device__ __forceinline__ void store_snapshot(const double2* row, int rank, bool live, double2* dst) {
    constexpr int TPR = RowCtx<N>::TPR, NE = 1 << (2 * N);
    if (live)
        for (int i = rank; i < NE; i += TPR) dst[i] = row[i];
    __syncthreads();
}

// The way back in two halves: a thread's 16 elements of a snapshot into registers (issued one unit ahead: the loads land
// while the unit in front of them is walked), and from there into the row's rho.
template <int N>
__device__ __forceinline__ void fetch_snapshot(double2 (&pf)[16], int rank, bool live, const double2* src) {
    constexpr int TPR = RowCtx<N>::TPR;
    if (live) {
#pragma unroll
        for (int k = 0; k < 16; ++k) pf[k] = src[rank + k * TPR];
    }
}

template <int N>
__device__ __forceinline__ void place_snapshot(double2* row, int rank, bool live, const double2 (&pf)[16]) {
    constexpr int TPR = RowCtx<N>::TPR;
    if (live) {
#pragma unroll
        for (int k = 0; k < 16; ++k) row[rank + k * TPR] = pf[k];
    }
    __syncthreads();
}

// density_dev_bwd_kernel with stored states: the forward sweep writes rho after every unit to a.snap and the reverse walk
// starts every unit from the stored state, so rho carries one unit's worth of inverse walk at most.  The text between the
// snapshot lines is that kernel's.  (As one body templated over `bool Stored` the inverse kernel's instantiations changed --
// one more scalar spill at n = 2, 3, 4, 6, profiles/r33_resource_usage.txt -- so the two kernels share the device functions
// above and nothing else.)
template <int N>
__global__ __launch_bounds__(bwd_threads<N>()) void density_dev_stored_bwd_kernel(DevStoredArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dens_lds[];      // rho, O, h'[D], the waves' trace partials
    using C = RowCtx<N>;
    constexpr int TPR = C::TPR, RPW = bwd_threads<N>() / TPR, D = 1 << N, NE = 1 << (2 * N);
    double2* state = reinterpret_cast<double2*>(dens_lds);
    double* hv = reinterpret_cast<double*>(dens_lds + 2 * RPW * NE * sizeof(double2));
    const int tid = threadIdx.x, slot = tid / TPR, rank = tid % TPR;
    long r = (long)blockIdx.x * RPW + slot;
    const bool live = r < a.B;
    if (!live) r = a.B - 1;                                              // a tail slot repeats the last row and stores nothing
    const double2* csr = a.cs + r * a.E;
    C cx;
    cx.rho = state + slot * NE;
    cx.obs = state + RPW * NE + slot * NE;
    cx.red = hv + D;
    cx.rank = rank; cx.sf = slot_fold<N>(slot); cx.parity = 0;
    cx.r = r; cx.B = a.B; cx.live = live;
    double2* row = cx.rho;
    const int sf = cx.sf;
    const long ustride = a.B * (long)NE;
    double2* snap = a.snap + r * (long)NE;                               // the row's snapshot of the unit the walk stands at
    int units = 0;

    // value table under the readout confusion: per bit, h'[k] = (1 - f) h[k] + f h[k ^ bit], f = P(the bit of k is misread)
    double h = 0.0;
    if (tid < D) h = a.diag ? a.diag[tid] : a.off + a.co * (double)(N - 2 * (int)__popc(tid));
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (tid < D) hv[tid] = h;
        __syncthreads();
        if (tid < D) {
            const double f = a.tab[i * kTabWire + kTabRead + ((tid >> i) & 1)];
            h = (1.0 - f) * h + f * hv[tid ^ (1 << i)];
        }
        __syncthreads();
    }
    if (tid < D) hv[tid] = h;

    // forward sweep: the passes of density_dev_fwd_kernel
    int s = 0, col = 0;
    bool first = true;
    for (int g = 0; g < 2; ++g) {
        for (int b = 0; b < a.nb[g]; ++b) {
            if (a.ld[g] == 0) {
                dev_enc_passes<N, 0>(row, rank, sf, a, csr, col, first);
                first = false;
                store_snapshot<N>(row, rank, live, snap); snap += ustride; ++units;
            }
            for (int l = 0; l < a.ld[g]; ++l, ++s) {
                dev_ring_passes<N, 0>(row, rank, sf, a, csr, s, col, l == 0, first);
                first = false;
                store_snapshot<N>(row, rank, live, snap); snap += ustride; ++units;
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
        double m1 = 0.0;
        for (int k = 0; k < D; ++k) {
            int i = 0;
#pragma unroll
            for (int w = 0; w < N; ++w) i |= ((k >> w) & 1) * (3 << (2 * w));
            m1 += row[i ^ fold(i) ^ sf].x * hv[k];
        }
        const double p = m1 + (a.bias ? a.bias[0] : 0.0);
        a.pred_ws[r] = p;
        if (a.pred) a.pred[r] = p;
    }

    // O = diag h' in the read-out basis
    for (int i = rank; i < NE; i += TPR) {
        int k = 0;
        bool diag = true;
#pragma unroll
        for (int w = 0; w < N; ++w) {
            const int rb = (i >> (2 * w)) & 1, cb = (i >> (2 * w + 1)) & 1;
            diag = diag && rb == cb;
            k |= rb << w;
        }
        cx.obs[i ^ fold(i) ^ sf] = make_double2(diag ? hv[k] : 0.0, 0.0);
    }
    __syncthreads();
    // back to the computational basis: O through the daggers of the basis change (rho is reloaded)
    if (a.pauli == QHEA_PAULI_X) basis_passes_back<N, 0, 3>(cx.obs, rank, sf);
    else if (a.pauli == QHEA_PAULI_Y) basis_passes_back<N, 0, 4>(cx.obs, rank, sf);

    // reverse walk: blocks, sub-layers and passes in reverse order; every unit starts from its stored state, fetched while
    // the unit behind it was walked
    double2 pf[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) pf[k] = make_double2(0.0, 0.0);
    if (units > 0) { snap -= ustride; fetch_snapshot<N>(pf, rank, live, snap); }
    auto open_unit = [&]() {
        place_snapshot<N>(cx.rho, rank, live, pf);
        if (--units > 0) { snap -= ustride; fetch_snapshot<N>(pf, rank, live, snap); }
    };
    for (int g = 1; g >= 0; --g) {
        for (int b = a.nb[g] - 1; b >= 0; --b) {
            col -= N;
            for (int l = a.ld[g] - 1; l >= 0; --l) {
                --s;
                open_unit();
                dev_ring_passes_back<N, N - 1>(cx, a, csr, s, col, l == 0);
            }
            if (a.ld[g] == 0) {
                open_unit();
                dev_enc_passes_back<N, 0>(cx, a, csr, col);
            }
        }
    }
}

// ---- host ----

// the kernel's table for a checked setting whose channels are all invertible
void fill_table(int n, const qhea_device_noise* dn, DevTable& t) {
    const DevSites sites(n, dn);
    for (int i = 0; i < kTabDoubles; ++i) t.v[i] = 0.0;
    for (int q = 0; q < n; ++q) {
        double* w = t.v + q * kTabWire;
        for (int k = 0; k < 4; ++k) {
            const Triple f = sites.at(k, q);
            double* c = w + k * kTabSite;
            element_form(f, c + 5 * kFormFwd);
            element_form(Triple{1.0 / f.off, 1.0 / f.a, -f.b / f.a}, c + 5 * kFormInv);
            element_form(f, c + 5 * kFormAdj);
            const double k01 = c[5 * kFormAdj + 2];                      // the adjoint's weight matrix is the transposed one
            c[5 * kFormAdj + 2] = c[5 * kFormAdj + 3]; c[5 * kFormAdj + 3] = k01;
        }
        slot_form(sites.lam2[q], w[kTabSlot], w[kTabSlot + 1]);
        w[kTabSlot + 2] = 1.0 / w[kTabSlot]; w[kTabSlot + 3] = -w[kTabSlot + 1] / w[kTabSlot];
        w[kTabRead] = dn->readout01[q]; w[kTabRead + 1] = dn->readout10[q];
    }
}

// The unit record of grad_loss_grad / grad_train_steps (hea_density_grad.hpp): the channel sites of a qhea_device_noise.  Its
// workspace is the uniform unit's with the table behind it.
struct DevGradUnit {
    using Noise = qhea_device_noise;
    static constexpr bool kStepCheckFirst = false;
    static size_t off_tab(const ModelInfo& mi, int64_t B) { return dens_grad_layout(mi, B).total; }
    static size_t workspace_bytes(const ModelInfo& mi, int64_t B) { return align256(off_tab(mi, B) + kTabDoubles * sizeof(double)); }
    // QHEA_EUNSUPPORTED for n >= 7 and for what the guard refuses, between the setting's checks and the shared ones (which get
    // an all-zero qhea_noise: the guard has been answered here)
    static int refuse(const ModelInfo& mi, const qhea_device_noise* dn) {
        if (mi.n > kDevMaxWires) return QHEA_EUNSUPPORTED;
        return device_log10_amplification(mi, dn) <= kMaxLog10AmplificationDevice ? QHEA_OK : QHEA_EUNSUPPORTED;
    }
    static int check(const qhea_model_desc* desc, const double* ham_diag, const qhea_device_noise* dn, int64_t count,
                     const double* trunk, std::initializer_list<const void*> required, void* workspace, void* stream,
                     NoisyCall& c) {
        return device_call_check({QHEA_MIN_QUBITS, kDevMaxWires /* 2 x 4^n elements per row in LDS */, false, false}, desc,
                                 ham_diag, dn, refuse, count, trunk, required, workspace, stream, c);
    }
    // the table, at its offset in a workspace for `bmax` rows
    static bool batch_ok(const ModelInfo&, int64_t) { return true; }
    static int once(const ModelInfo& mi, const qhea_device_noise* dn, char* ws, int64_t bmax, hipStream_t st) {
        DevTable t;
        fill_table(mi.n, dn, t);
        hipLaunchKernelGGL(dev_table_kernel, dim3(1), dim3(64), 0, st, t, reinterpret_cast<double*>(ws + off_tab(mi, bmax)));
        return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
    }
    static int launch_bwd(const GradBatch& b, const qhea_device_noise*) {
        DevGradArgs a{};
        circuit_args(a, b.desc, b.mi, b.params, b.ham_diag, b.batch, b.gates, b.cs);
        a.tab = reinterpret_cast<const double*>(b.ws + off_tab(b.mi, b.bmax));
        a.w = b.params + b.mi.off_ans;
        a.pred = b.pred; a.pred_ws = b.pred_ws; a.rec = b.rec;
        return dispatch_n(b.mi.n, [&](auto n) { return launch_density_bwd<n()>(density_dev_bwd_kernel<n()>, a.B, a, b.st); });
    }
};

// The unit record of the stored-state calls: DevGradUnit with the snapshot region behind its workspace, the guard asked of the
// largest single unit (between two stored states rho walks back through one unit, and one unit is a circuit of the kind the
// bound was measured on), and the stored-state kernel.  Table, prep and reduce launches are the inverse unit's.
struct DevStoredGradUnit : DevGradUnit {
    // U: sub-layers, plus the blocks without any (one encoding-only unit each)
    static size_t units(const ModelInfo& mi) {
        size_t u = 0;
        for (int g = 0; g < 2; ++g) u += (size_t)mi.nb[g] * (size_t)(mi.ld[g] == 0 ? 1 : mi.ld[g]);
        return u;
    }
    static size_t off_snap(const ModelInfo& mi, int64_t B) { return DevGradUnit::workspace_bytes(mi, B); }
    static size_t workspace_bytes(const ModelInfo& mi, int64_t B) {
        return off_snap(mi, B) + align256(units(mi) * (size_t)B * (sizeof(double2) << (2 * mi.n)));
    }
    static int refuse(const ModelInfo& mi, const qhea_device_noise* dn) {
        if (mi.n > kDevMaxWires) return QHEA_EUNSUPPORTED;
        return device_log10_amplification(mi, dn, true) <= kMaxLog10AmplificationDevice ? QHEA_OK : QHEA_EUNSUPPORTED;
    }
    static int check(const qhea_model_desc* desc, const double* ham_diag, const qhea_device_noise* dn, int64_t count,
                     const double* trunk, std::initializer_list<const void*> required, void* workspace, void* stream,
                     NoisyCall& c) {
        return device_call_check({QHEA_MIN_QUBITS, kDevMaxWires, false, false}, desc, ham_diag, dn, refuse, count, trunk, required,
                                 workspace, stream, c);
    }
    static int launch_bwd(const GradBatch& b, const qhea_device_noise*) {
        DevStoredArgs a{};
        circuit_args(a, b.desc, b.mi, b.params, b.ham_diag, b.batch, b.gates, b.cs);
        a.tab = reinterpret_cast<const double*>(b.ws + off_tab(b.mi, b.bmax));
        a.w = b.params + b.mi.off_ans;
        a.pred = b.pred; a.pred_ws = b.pred_ws; a.rec = b.rec;
        a.snap = reinterpret_cast<double2*>(b.ws + off_snap(b.mi, b.bmax));
        return dispatch_n(b.mi.n, [&](auto n) { return launch_density_bwd<n()>(density_dev_stored_bwd_kernel<n()>, a.B, a, b.st); });
    }
};

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_device_noisy_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    return grad_workspace_bytes<DevGradUnit>(desc, batch);
}

double qhea_model_device_noisy_log10_amplification(const qhea_model_desc* desc, const qhea_device_noise* dn) {
    ModelInfo mi;
    if (model_info(desc, mi) != QHEA_OK || device_noise_check(mi.n, dn) != QHEA_OK) return NAN;
    return device_log10_amplification(mi, dn);
}

int qhea_model_loss_grad_noisy_device_exact(const qhea_model_desc* desc, int64_t batch, const double* branch,
                                            const double* trunk, const double* y, const double* params, const double* ham_diag,
                                            const qhea_device_noise* dn, double inv_batch_total, double* grad, double* pred,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    return grad_loss_grad<DevGradUnit>(desc, batch, branch, trunk, y, params, ham_diag, dn, inv_batch_total, grad, pred, workspace,
                                       workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_device_exact(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                              const double* branch, const double* trunk, const double* y, double* params,
                                              const double* ham_diag, const qhea_device_noise* dn,
                                              const double* inv_batch_total, double* grad, int64_t grad_stride, double* exp_avg,
                                              double* exp_avg_sq, int64_t first_step, double lr, double beta1, double beta2,
                                              double eps, double weight_decay, void* workspace, size_t workspace_bytes,
                                              void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return grad_train_steps<DevGradUnit>(desc, call, ham_diag, dn, lr);
}

size_t qhea_model_device_noisy_stored_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    return grad_workspace_bytes<DevStoredGradUnit>(desc, batch);
}

double qhea_model_device_noisy_log10_layer_amplification(const qhea_model_desc* desc, const qhea_device_noise* dn) {
    ModelInfo mi;
    if (model_info(desc, mi) != QHEA_OK || device_noise_check(mi.n, dn) != QHEA_OK) return NAN;
    return device_log10_amplification(mi, dn, true);
}

int qhea_model_loss_grad_noisy_device_exact_stored(const qhea_model_desc* desc, int64_t batch, const double* branch,
                                                   const double* trunk, const double* y, const double* params,
                                                   const double* ham_diag, const qhea_device_noise* dn, double inv_batch_total,
                                                   double* grad, double* pred, void* workspace, size_t workspace_bytes,
                                                   void* stream) {
    return grad_loss_grad<DevStoredGradUnit>(desc, batch, branch, trunk, y, params, ham_diag, dn, inv_batch_total, grad, pred,
                                             workspace, workspace_bytes, stream);
}

int qhea_model_train_steps_noisy_device_exact_stored(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                                     const double* branch, const double* trunk, const double* y, double* params,
                                                     const double* ham_diag, const qhea_device_noise* dn,
                                                     const double* inv_batch_total, double* grad, int64_t grad_stride,
                                                     double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr,
                                                     double beta1, double beta2, double eps, double weight_decay, void* workspace,
                                                     size_t workspace_bytes, void* stream) {
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return grad_train_steps<DevStoredGradUnit>(desc, call, ham_diag, dn, lr);
}

}  // extern "C"
