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
#include <vector>

#include "hea_density_grad.hpp"
#include "hea_device_noise.hpp"
#include "hea_train.hpp"
#include "hea_sincos.hpp"

namespace qhea {
namespace {

// table of one wire q (doubles): [site][form][off, k00, k01, k10, k11], then the slot q's D2 and the wire's readout
constexpr int kFormFwd = 0, kFormInv = 1, kFormAdj = 2;
constexpr int kTabSite = 15, kTabSlot = 60 /* keep2, mix2, inverse keep2, inverse mix2 */, kTabRead = 64 /* r01, r10 */;
constexpr int kTabWire = 66, kTabDoubles = kTabWire * kDevMaxWires;

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

// A scalar zero the compiler cannot see through: a table address formed behind it belongs to the pass that forms it, so the
// loads of a pass' constants are neither hoisted ahead of the loop over the sub-layers nor shared between passes.
__device__ __forceinline__ int opaque_szero() {
    int z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    return z;
}

// one table entry in scalar registers (the address is the same in every lane)
__device__ __forceinline__ double uniform_load(const double* p) {
    const double v = *p;
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// the 2 x 2 blocks of one wire under the five constants at c: (off, k00, k01, k10, k11)
template <int S>
__device__ __forceinline__ void channel5(double2 (&e)[16], const double* c) {
    const double off = uniform_load(c), k00 = uniform_load(c + 1), k01 = uniform_load(c + 2), k10 = uniform_load(c + 3),
                 k11 = uniform_load(c + 4);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int b = S == 1 ? 4 * m : m;
        const double2 d0 = e[b], d1 = e[b + 3 * S];
        e[b] = make_double2(k00 * d0.x + k01 * d1.x, k00 * d0.y + k01 * d1.y);
        e[b + 3 * S] = make_double2(k10 * d0.x + k11 * d1.x, k10 * d0.y + k11 * d1.y);
        e[b + S].x *= off; e[b + S].y *= off;
        e[b + 2 * S].x *= off; e[b + 2 * S].y *= off;
    }
}

__device__ __forceinline__ const double* site_at(const double* tab, int q, int site, int form) {
    return tab + q * kTabWire + site * kTabSite + form * 5;
}

// ---- forward sweep: the passes of density_dev_fwd_kernel with the constants read from the table ----
// dev_wire_gates, dev_cnot_depolarize2, dev_ring_passes and dev_enc_passes below are hea_density_device.hip's functions of the
// same names, statement for statement; only where a site's constants come from differs (there: members of the by-value
// argument indexed at compile time; here: the workspace table, loaded inside the pass).  A change to the forward model is
// made in both; tests/test_device_noise_training.py holds this sweep's pred to the forward call's within 1e-13.

template <int N, int S>
__device__ __forceinline__ void dev_wire_gates(double2 (&e)[16], const DevGradArgs& a, const double* tab, const double2* csr,
                                               int s, int col, bool enc, int q) {
    if (enc) {
        const double2 c = csr[col + q];
        apply_gate<S>(e, U2{{c.x, 0.0}, {0.0, -c.y}, {0.0, -c.y}, {c.x, 0.0}});
        channel5<S>(e, site_at(tab, q, kEnc, kFormFwd));
    }
    const double4 v = a.gates[2 * (s * N + q + N)];                      // (u00, u01); u10 = -conj(u01), u11 = conj(u00)
    apply_gate<S>(e, U2{{v.x, v.y}, {v.z, v.w}, {-v.z, v.w}, {v.x, -v.y}});
    channel5<S>(e, site_at(tab, q, kRot, kFormFwd));
}

// CNOT(c -> t) on both indices, then the two-qubit channel (keep, mix)
__device__ __forceinline__ void dev_cnot_depolarize2(double2 (&e)[16], double keep, double mix) {
    double2 r[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) r[k] = e[k ^ ((k >> 2) & 1) ^ (((k >> 3) & 1) << 1)];
    const double sx = (r[0].x + r[3].x) + (r[12].x + r[15].x), sy = (r[0].y + r[3].y) + (r[12].y + r[15].y);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool eq = k == 0 || k == 3 || k == 12 || k == 15;          // row bits (c, t) = column bits
        e[k].x = eq ? keep * r[k].x + mix * sx : keep * r[k].x;
        e[k].y = eq ? keep * r[k].y + mix * sy : keep * r[k].y;
    }
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
        dev_cnot_depolarize2(e, uniform_load(tab + J * kTabWire + kTabSlot), uniform_load(tab + J * kTabWire + kTabSlot + 1));
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
        apply_gate<1>(e, U2{{c0.x, 0.0}, {0.0, -c0.y}, {0.0, -c0.y}, {c0.x, 0.0}});
        channel5<1>(e, site_at(tab, P::t, kEnc, kFormFwd));
        if (J + 1 < N) {
            const double2 c1 = csr[col + P::c];
            apply_gate<4>(e, U2{{c1.x, 0.0}, {0.0, -c1.y}, {0.0, -c1.y}, {c1.x, 0.0}});
            channel5<4>(e, site_at(tab, P::c, kEnc, kFormFwd));
        }
        P::store(e, row, b);
        __syncthreads();
        dev_enc_passes<N, J + 2>(row, rank, sf, a, csr, col, false);
    }
}

// ---- reverse walk ----

// site `site` of wire q in reverse: its inverse on rho, its adjoint on O
template <int S>
__device__ __forceinline__ void undo_site(double2 (&e)[16], double2 (&o)[16], const double* tab, int q, int site) {
    channel5<S>(e, site_at(tab, q, site, kFormInv));
    channel5<S>(o, site_at(tab, q, site, kFormAdj));
}

// encoding of wire q: its site, trace (slot 3 of the wire's four), RX^dagger
template <int S>
__device__ __forceinline__ void dev_undo_encoding(double2 (&e)[16], double2 (&o)[16], const double* tab, int q, double2 c,
                                                  double* tr) {
    undo_site<S>(e, o, tab, q, kEnc);
    tr[3] = pinned(trace16<S, 0>(o, e));
    unrotate_x<S>(e, c.x, c.y);
    unrotate_x<S>(o, c.x, c.y);
}

// wire q's gates of sub-layer s in reverse; tr[k] = this thread's share of d pred / d w[s, k, q], tr[3] of d pred / d x[col + q]
template <int N, int S>
__device__ __forceinline__ void dev_undo_wire(double2 (&e)[16], double2 (&o)[16], const DevGradArgs& a, const double* tab,
                                              const double2* csr, int s, int col, bool enc, int q, double* tr) {
    undo_site<S>(e, o, tab, q, kRot);
    const double* ws = a.w + (long)s * 3 * N + q;
    double sn, cn;
    tr[2] = pinned(trace16<S, 1>(o, e));
    fast_sincos(0.5 * ws[2 * N], &sn, &cn);
    unrotate_y<S>(e, cn, sn);
    unrotate_y<S>(o, cn, sn);
    tr[1] = pinned(trace16<S, 2>(o, e));
    fast_sincos(0.5 * ws[N], &sn, &cn);
    unrotate_z<S>(e, cn, sn); unrotate_z<S>(o, cn, sn);
    tr[0] = pinned(trace16<S, 1>(o, e));
    fast_sincos(0.5 * ws[0], &sn, &cn);
    unrotate_y<S>(e, cn, sn);
    unrotate_y<S>(o, cn, sn);
    tr[3] = 0.0;
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

template <int N>
int launch_density_dev_bwd(const DevGradArgs& a, hipStream_t st) {
    constexpr int T = bwd_threads<N>(), TPR = 1 << (2 * N - 4), RPW = T / TPR, WPR = TPR > 64 ? TPR / 64 : 1;
    constexpr size_t smem = 2 * (size_t)RPW * (1 << (2 * N)) * sizeof(double2) + (1 << N) * sizeof(double) +
                            2 * WPR * kTracesPerPass * sizeof(double);
    return launch_dynamic_lds(density_dev_bwd_kernel<N>, dim3((unsigned)((a.B + RPW - 1) / RPW)), dim3(T), smem, st, a);
}

// ---- host ----

// the element form (off, k00, k01, k10, k11) of a triple
void element_form(const Triple& t, double* c) {
    c[0] = t.off;
    c[1] = 0.5 * (1.0 + t.a + t.b); c[2] = 0.5 * (1.0 - t.a + t.b);
    c[3] = 0.5 * (1.0 - t.a - t.b); c[4] = 0.5 * (1.0 + t.a - t.b);
}

// the kernel's table for a checked setting whose channels are all invertible
void fill_table(int n, const qhea_device_noise* dn, DevTable& t) {
    double chan[4][kDevMaxWires][3] = {}, lam2[kDevMaxWires] = {};
    device_noise_compose(n, dn, &chan[0][0][0], kDevMaxWires, lam2);
    for (int i = 0; i < kTabDoubles; ++i) t.v[i] = 0.0;
    for (int q = 0; q < n; ++q) {
        double* w = t.v + q * kTabWire;
        for (int k = 0; k < 4; ++k) {
            const Triple f{chan[k][q][0], chan[k][q][1], chan[k][q][2]};
            double* c = w + k * kTabSite;
            element_form(f, c + 5 * kFormFwd);
            element_form(Triple{1.0 / f.off, 1.0 / f.a, -f.b / f.a}, c + 5 * kFormInv);
            element_form(f, c + 5 * kFormAdj);
            const double k01 = c[5 * kFormAdj + 2];                      // the adjoint's weight matrix is the transposed one
            c[5 * kFormAdj + 2] = c[5 * kFormAdj + 3]; c[5 * kFormAdj + 3] = k01;
        }
        const double keep = 1.0 - lam2[q];
        w[kTabSlot] = keep; w[kTabSlot + 1] = 0.25 * lam2[q];
        w[kTabSlot + 2] = 1.0 / keep; w[kTabSlot + 3] = -0.25 * lam2[q] / keep;
        w[kTabRead] = dn->readout01[q]; w[kTabRead + 1] = dn->readout10[q];
    }
}

// log10 A_dev of a checked setting: - sum log10 min(off, a) over the one-wire sites the circuit applies (ENC once per block,
// ROT / CTL / TGT once per sub-layer) - sum log10 (1 - lam_j) over its CNOT slots; +inf for a singular channel
double device_log10_amplification(const ModelInfo& mi, const qhea_device_noise* dn) {
    const int n = mi.n;
    for (int q = 0; q < n; ++q)
        if (!(dn->p1[q] < 0.75) || !(dn->p2[q] < 15.0 / 16.0)) return INFINITY;
    std::vector<double> chan((size_t)4 * n * 3), lam2((size_t)n);
    device_noise_compose(n, dn, chan.data(), n, lam2.data());
    const double count[4] = {(double)(mi.sh.E / n), (double)mi.sh.blk, (double)mi.sh.blk, (double)mi.sh.blk};
    double sum = 0.0;
    for (int k = 0; k < 4; ++k) {
        if (count[k] == 0.0) continue;
        for (int q = 0; q < n; ++q) {
            const double* c = chan.data() + ((size_t)k * n + q) * 3;
            const double m = c[0] < c[1] ? c[0] : c[1];
            if (!(m > 0.0)) return INFINITY;
            sum -= count[k] * log10(m);
        }
    }
    for (int j = 0; j < n && mi.sh.blk > 0; ++j) sum -= (double)mi.sh.blk * log10(1.0 - lam2[j]);
    return sum;
}

// The guard's bound on log10 A_dev.  The uniform walk's 12 (kMaxLog10Amplification) does not carry over: a site with b != 0 is
// not self-adjoint, O no longer shrinks by the factor rho grows by, and the numpy probe of tests/test_device_noise_training_abi.py
// (inverse walk against a walk over stored forward states; n = 5 with 60 and 120 sub-layers, n = 6 with 20) shows at most
// 2.1e-15 at log10 A_dev = 4, 1.3e-14 at 5, 4.5e-14 at 6, 2.4e-13 at 7, but 1.5e-12 at 8 and 1.1e-9 at 11.99.  7 is the
// largest probed value that stays under the 1e-12 the uniform bound was held to.
constexpr double kMaxLog10AmplificationDevice = 7.0;

struct DevGradLayout { DensGradLayout g; size_t off_tab, total; };

DevGradLayout dev_grad_layout(const ModelInfo& mi, int64_t B) {
    DevGradLayout L{};
    L.g = dens_grad_layout(mi, B);
    L.off_tab = L.g.total;
    L.total = align256(L.off_tab + kTabDoubles * sizeof(double));
    return L;
}

constexpr NoisyKind kDevGradKind{QHEA_MIN_QUBITS, kDevMaxWires /* 2 x 4^n elements per row in LDS */, false, false};

// What opens both calls, in the order the ABI reports it: the descriptor, the setting's QHEA_EINVAL cases (the forward device
// call's checking code), QHEA_EUNSUPPORTED for n >= 7 and the guard, then the shared checks of the uniform gradient call (which
// get an all-zero qhea_noise: the guard has been answered here).  The model is read into a record of its own first, as in
// hea_density_device.hip: model_info appends to the record's block list.
int dev_grad_check(const qhea_model_desc* desc, const double* ham_diag, const qhea_device_noise* dn, int64_t count,
                   const double* trunk, std::initializer_list<const void*> required, void* workspace, void* stream,
                   NoisyCall& c) {
    ModelInfo probe;
    int rc = model_info(desc, probe);
    if (rc != QHEA_OK) return rc;
    rc = device_noise_check(probe.n, dn);
    if (rc != QHEA_OK) return rc;
    if (probe.n > kDevMaxWires) return QHEA_EUNSUPPORTED;
    if (!(device_log10_amplification(probe, dn) <= kMaxLog10AmplificationDevice)) return QHEA_EUNSUPPORTED;
    const qhea_noise none{};
    return noisy_call_check(kDevGradKind, desc, ham_diag, &none, 0, count, trunk, required, workspace, stream, c);
}

int launch_dev_table(const ModelInfo& mi, const qhea_device_noise* dn, char* ws, int64_t bmax, hipStream_t st) {
    DevTable t;
    fill_table(mi.n, dn, t);
    hipLaunchKernelGGL(dev_table_kernel, dim3(1), dim3(64), 0, st, t, reinterpret_cast<double*>(ws + dev_grad_layout(mi, bmax).off_tab));
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

// prep, density backward, reduce (+ Adam when adam.p) for one batch; the arguments have been checked and the table (at the
// offset of a workspace for `bmax` rows) written
int dev_loss_grad_launch(const qhea_model_desc* desc, const ModelInfo& mi, int64_t batch, int64_t bmax, const double* branch,
                         const double* trunk, const double* y, const double* params, const double* ham_diag, double inv_bt,
                         double* grad, double* pred, char* ws, hipStream_t st, const AdamArgs& adam) {
    const DensGradLayout L = dens_grad_layout(mi, batch);
    double4* gates = reinterpret_cast<double4*>(ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(ws + L.off_cs);
    int rc = launch_prep_model(desc, mi, batch, branch, trunk, params, gates, cs, ws, st);
    if (rc != QHEA_OK) return rc;

    DevGradArgs a{};
    a.gates = gates; a.cs = cs; a.diag = ham_diag;
    a.bias = mi.has_bias ? params + mi.off_bias : nullptr;
    a.tab = reinterpret_cast<const double*>(ws + dev_grad_layout(mi, bmax).off_tab);
    a.w = params + mi.off_ans;
    a.off = desc->ham_offset; a.co = desc->ham_coeff;
    a.B = batch; a.E = (int)mi.sh.E; a.pauli = desc->ham_pauli;
    for (int g = 0; g < 2; ++g) { a.nb[g] = mi.nb[g]; a.ld[g] = mi.ld[g]; }
    a.pred = pred;
    a.pred_ws = reinterpret_cast<double*>(ws + L.off_pred);
    a.rec = reinterpret_cast<double*>(ws + L.off_rec);
    switch (mi.n) {
        case 2: rc = launch_density_dev_bwd<2>(a, st); break;
        case 3: rc = launch_density_dev_bwd<3>(a, st); break;
        case 4: rc = launch_density_dev_bwd<4>(a, st); break;
        case 5: rc = launch_density_dev_bwd<5>(a, st); break;
        case 6: rc = launch_density_dev_bwd<6>(a, st); break;
        default: rc = QHEA_EUNSUPPORTED;
    }
    if (rc != QHEA_OK) return rc;
    return launch_density_reduce(desc, mi, batch, branch, trunk, y, a.rec, a.pred_ws, inv_bt, grad, adam, st);
}

}  // namespace
}  // namespace qhea

using namespace qhea;

extern "C" {

size_t qhea_model_device_noisy_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (batch < 0 || model_info(desc, mi) != QHEA_OK) return 0;
    return dev_grad_layout(mi, batch).total;
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
    NoisyCall c;
    int rc = dev_grad_check(desc, ham_diag, dn, batch, trunk, {branch, y, params, grad}, workspace, stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    if (!workspace || workspace_bytes < dev_grad_layout(c.mi, batch).total) return QHEA_EWORKSPACE;
    rc = launch_dev_table(c.mi, dn, c.ws, batch, c.st);
    if (rc != QHEA_OK) return rc;
    return dev_loss_grad_launch(desc, c.mi, batch, batch, branch, trunk, y, params, ham_diag, inv_batch_total, grad, pred, c.ws,
                                c.st, AdamArgs{});
}

int qhea_model_train_steps_noisy_device_exact(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                                              const double* branch, const double* trunk, const double* y, double* params,
                                              const double* ham_diag, const qhea_device_noise* dn,
                                              const double* inv_batch_total, double* grad, int64_t grad_stride, double* exp_avg,
                                              double* exp_avg_sq, int64_t first_step, double lr, double beta1, double beta2,
                                              double eps, double weight_decay, void* workspace, size_t workspace_bytes,
                                              void* stream) {
    NoisyCall c;
    int rc = dev_grad_check(desc, ham_diag, dn, n_steps, trunk,
                            {row_begin, inv_batch_total, branch, y, grad, params, exp_avg, exp_avg_sq}, workspace, stream, c);
    if (rc != QHEA_OK) return rc;
    if (first_step < 1) return QHEA_EINVAL;
    if (c.empty) return QHEA_OK;
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    const int64_t bmax = call_max_batch(call, c.mi.P, *desc);
    if (bmax < 0) return QHEA_EINVAL;
    if (!workspace || workspace_bytes < dev_grad_layout(c.mi, bmax).total) return QHEA_EWORKSPACE;     // (every region grows with the batch)
    rc = launch_dev_table(c.mi, dn, c.ws, bmax, c.st);
    if (rc != QHEA_OK) return rc;
    for (int64_t i = 0; i < n_steps; ++i) {
        const StepView v = step_view(call, i, *desc);
        rc = dev_loss_grad_launch(desc, c.mi, v.nb, bmax, v.branch, v.trunk, v.y, params, ham_diag, v.inv_bt, v.grad, nullptr,
                                  c.ws, c.st, adam_step(call, i, lr).adam);
        if (rc != QHEA_OK) return rc;
    }
    return QHEA_OK;
}

}  // extern "C"
