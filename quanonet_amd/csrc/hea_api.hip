// hea_api.hip -- C ABI (include/quanonet_hea.h) of the MI355X HEA simulator: argument checks,
// workspace layout, the batch-invariant prep / reduce kernels and the per-qubit-count dispatch.
#include <atomic>
#include <cmath>
#include <algorithm>
#include <limits>
#include <vector>

#include "hea_device.hpp"
#include "hea_zyz.hpp"
#include "hea_sincos.hpp"
#include "hea_adam.hpp"
#include "hea_dp.hpp"
#include "hea_qsweep.hpp"
#include "hea_model.hpp"
#include "hea_train.hpp"

namespace qhea {

// Gate table entry g = s*n+q (64 B): U = RY(w[s,2,q]) RZ(w[s,1,q]) RY(w[s,0,q]) = [[a,b],[-conj b,conj a]]
// stored as two lane variants (ar, ai, br, bi) and (ar, -ai, -br, bi); `gates` points at entry -n
// (n identity entries of padding on each side).  cs[b,e] = (cos, sin)(x[b,e]/2).
// First 256 bytes of every workspace.  The caller's buffer arrives uninitialised, so the prep kernel that opens each
// call (stream-ordered before everything else) stamps the magic and zeroes the status the first time it sees the
// buffer; after that the status word is sticky until qhea_check_status() reads and clears it.
struct WorkspaceHeader {
    unsigned long long magic;
    int status;                    // OR of kStatus* bits
    int pad;
};
constexpr unsigned long long kWsMagic = 0x51484541'57530001ull;      // "QHEAWS" + layout version
__device__ __forceinline__ void header_init(WorkspaceHeader* h) {
    if (h->magic != kWsMagic) { h->status = 0; h->pad = 0; h->magic = kWsMagic; }
}

__global__ void prep_kernel(int n, int blk, const double* __restrict__ w, double4* __restrict__ gates,
                            long BE, const double* __restrict__ x, double2* __restrict__ cs, WorkspaceHeader* hdr) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid == 0) header_init(hdr);
    const long ng = (long)(blk + 2) * n;
    if (tid < ng) {
        const long g = tid - n;                       // real gate index, or padding
        double4 v0 = make_double4(1.0, 0.0, 0.0, 0.0);
        if (g >= 0 && g < (long)blk * n) {
            const int s = (int)(g / n), q = (int)(g % n);
            const double* ws = w + (long)s * 3 * n;
            double sa, ca, sb, cb, sc, cc;
            fast_sincos(0.5 * ws[q], &sa, &ca);
            fast_sincos(0.5 * ws[n + q], &sb, &cb);
            fast_sincos(0.5 * ws[2 * n + q], &sc, &cc);
            // M = RZ(b) RY(a): M00 = e^{-ib/2} ca, M01 = -e^{-ib/2} sa, M10 = e^{+ib/2} sa, M11 = e^{+ib/2} ca
            const double m00r = cb * ca, m00i = -sb * ca;
            const double m01r = -cb * sa, m01i = sb * sa;
            const double m10r = cb * sa, m10i = sb * sa;
            const double m11r = cb * ca, m11i = sb * ca;
            // U = RY(c) M: U00 = cc M00 - sc M10, U01 = cc M01 - sc M11
            v0 = make_double4(cc * m00r - sc * m10r, cc * m00i - sc * m10i,
                              cc * m01r - sc * m11r, cc * m01i - sc * m11i);
        }
        gates[2 * tid] = v0;
        gates[2 * tid + 1] = make_double4(v0.x, -v0.y, -v0.z, v0.w);
    } else if (tid - ng < BE) {
        const long t = tid - ng;
        double s, c;
        fast_sincos(0.5 * x[t], &s, &c);
        cs[t] = make_double2(c, s);
    }
}

// ---------------------------------------------------------------------------------------
// ZYZ form of the fused ansatz gate (hea_zyz.hpp):  RY(c) RZ(b) RY(a) = RZ(alpha) RY(theta) RZ(beta) exactly (both sides
// are the same SU(2) matrix [[A, B], [-conj B, conj A]], A = cos(theta/2) e^{-i(alpha+beta)/2}, B = -sin(theta/2) e^{-i(alpha-beta)/2}).
// Everything is done on unit phasors -- no atan2, no angle wrap: p = A/|A|, m = -B/|B|, e^{-i alpha} = p m,
// u = e^{-i alpha/2} = sqrt(p m) (either branch), v = e^{-i beta/2} = p conj(u)  (then u v = p and u conj(v) = m).
// A vanishing |A| or |B| leaves one phasor free: any choice reproduces the matrix, because the phasor only ever
// multiplies the vanishing modulus.
// ---------------------------------------------------------------------------------------
// Diagnostic build (-DQHEA_REDUCE_STAMPS, scripts/exp/reduce_stamps.py): thread 0 of reduce block 30 notes the shader clock at
// the phases of the reduce kernel and prints the differences at its end.
#ifdef QHEA_REDUCE_STAMPS
__device__ unsigned long long qhea_stamps[16];
#define QHEA_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 30) qhea_stamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define QHEA_STAMP(i) do {} while (0)
#endif
struct GateZ {
    double c, s;        // cos(theta/2), sin(theta/2) >= 0
    double2 u, v;       // e^{-i alpha/2}, e^{-i beta/2}
    double cosb, sinb, cosc, sinc;      // of the FULL angles b = w[s,1,q], c = w[s,2,q] (gradient map of the reduce kernel)
};
// (The prep / reduce code below is inlined into several kernels whose results are compared BITWISE -- records written by
// prep_zyz_kernel or by the reduce kernel, gradients through reduce_kernel or any reduce_model_kernel instantiation -- so it
// does not leave the choice of fused multiply-adds to the compiler: implicit contraction is off, the FMAs that matter are
// written out.)
__device__ __forceinline__ double2 cmul(const double2& a, const double2& b) {
#pragma clang fp contract(off)
    return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ double2 cconj(const double2& a) { return make_double2(a.x, -a.y); }
// (cos, sin) of the three HALF angles a/2, b/2, c/2 of the gate, computed by three threads (prep_zyz_kernel)
__device__ inline GateZ gate_zyz(const double2& ha, const double2& hb, const double2& hc) {
#pragma clang fp contract(off)
    const double ca = ha.x, sa = ha.y, cb = hb.x, sb = hb.y, cc = hc.x, sc = hc.y;
    const double m00r = cb * ca, m00i = -sb * ca, m01r = -cb * sa, m01i = sb * sa;
    const double m10r = cb * sa, m10i = sb * sa, m11r = cb * ca, m11i = sb * ca;
    const double Ar = cc * m00r - sc * m10r, Ai = cc * m00i - sc * m10i;
    const double Br = cc * m01r - sc * m11r, Bi = cc * m01i - sc * m11i;
    // moduli and phasors through reciprocal square roots (3 rsqrt instead of 4 sqrt + 7 divisions in a row: this function is
    // on the critical path of the reduce kernel that writes the next step's records).  |A|^2 + |B|^2 = 1 up to rounding (the
    // matrix is a product of three rotations), so cos(theta/2) = |A|, sin(theta/2) = |B| need no further normalisation.
    const double a2 = Ar * Ar + Ai * Ai, b2 = Br * Br + Bi * Bi;
    const double ia = rsqrt(a2), ib = rsqrt(b2);
    GateZ g;
    g.c = a2 > 0.0 ? a2 * ia : 0.0; g.s = b2 > 0.0 ? b2 * ib : 0.0;
    const double2 p = a2 > 0.0 ? make_double2(Ar * ia, Ai * ia) : make_double2(1.0, 0.0);
    const double2 m = b2 > 0.0 ? make_double2(-Br * ib, -Bi * ib) : make_double2(1.0, 0.0);
    const double2 z = cmul(p, m);
    // u = sqrt(z) on the unit circle: with t = (1 + |Re z|) / 2 >= 1/2, the larger component is sqrt(t), the other Im z / (2 sqrt(t))
    const double t = 0.5 * (1.0 + fabs(z.x)), it = rsqrt(t);
    const double big = t * it, small = 0.5 * z.y * it;
    double2 u;
    if (z.x >= 0.0) { u.x = big; u.y = small; }
    else            { u.y = copysign(big, z.y); u.x = fabs(small); }
    g.u = u;
    g.v = cmul(p, cconj(u));
    g.cosb = cb * cb - sb * sb; g.sinb = 2.0 * sb * cb;
    g.cosc = cc * cc - sc * sc; g.sinc = 2.0 * sc * cc;
    return g;
}

// Tangent form of the split records' RY part (hea_zyz.hpp, SplitCoef): per wire q < 4 the gate's t = s / c, and the
// sub-layer's scale P = c0 c1 c2 c3 that wire 4's coefficients carry.  A cosine below 2^-100 in magnitude is replaced by
// +-2^-100 first (sign kept, +0 -> +): that moves the state by < 1e-30 and keeps t, and four such gates' P t's, finite.
// ONE definition for every kernel that writes records (they are compared bitwise): the same operands in the same order.
__device__ __forceinline__ double tan_cos(double c) {
    constexpr double kTiny = 0x1p-100;
    return fabs(c) < kTiny ? (signbit(c) ? -kTiny : kTiny) : c;
}
__device__ __forceinline__ double tan_t(const GateZ& g) {
#pragma clang fp contract(off)
    return g.s / tan_cos(g.c);
}
__device__ __forceinline__ double tan_scale(const GateZ* z /* the sub-layer's five gates */) {
#pragma clang fp contract(off)
    return (tan_cos(z[0].c) * tan_cos(z[1].c)) * (tan_cos(z[2].c) * tan_cos(z[3].c));
}

// source index of the CNOT ring as a permutation of basis indices (n <= 5): after the ring, amplitude k is the old
// amplitude ring_src_index(n, k)  (== ring_source<N>(lane, false) >> 2 of hea_device.hpp)
__device__ __forceinline__ int ring_src_index(int n, int k) {
    for (int i = n - 1; i >= 0; --i) k ^= ((k >> ((i + 1) % n)) & 1) << i;
    return k;
}
struct LayerInfo { int kind; int s; int m; };      // kind 0: RX chunk of m gates, 1: ansatz sub-layer s, 2: none
__device__ inline LayerInfo decode_layer(const Runs& r, int n, int l) {
    LayerInfo none{2, 0, 0};
    if (l < 0) return none;
    int s_base = 0;
    for (int i = 0; i < r.nruns; ++i) {
        const int nch = (r.enc[i] + n - 1) / n, per = nch + r.ld[i];
        const long tot = (long)per * r.count[i];
        if (l < tot) {
            const int rep = l / per, idx = l % per;
            if (idx < nch) {
                const int left = r.enc[i] - idx * n;
                return LayerInfo{0, 0, left < n ? left : n};
            }
            return LayerInfo{1, s_base + rep * r.ld[i] + (idx - nch), 0};
        }
        l -= (int)tot;
        s_base += r.ld[i] * r.count[i];
    }
    return none;
}

// One 64-thread block per layer record l = 0 .. L (hea_zyz.hpp): thread k < 2^n writes the diagonal entry
//   e^{i Phi_l(k)} = prod_q [pre-diagonal RZ(beta_q) of layer l, if it is an ansatz sub-layer]
//                  x prod_q [post-diagonal RZ(alpha_q) of layer l-1, if THAT is an ansatz sub-layer, seen through its ring];
// threads 32 .. 32+2n write the RY coefficients of an ansatz layer.  Native RX chunks have no diagonals of their own.
// It also leaves, per ansatz gate, the six numbers the reduce kernel's gradient map needs (cos/sin of b, c and alpha),
// so that the reduce kernel does not spend five serial sincos per gate on them: gmap[s*n + q] = 8 doubles.
constexpr int kGmapDoubles = 8;
struct PrepShared {
    GateZ gz[2][QHEA_MAX_QUBITS];           // [0]: this layer's gates, [1]: the previous layer's
    double2 half[2][3][QHEA_MAX_QUBITS];    // (cos, sin) of the half angles: one sincos per thread, not three in a row
};
// What the decomposition of gate (s, q) of ansatz sub-layer s = layer l leaves in memory besides its GateZ: the reduce kernel's
// gradient-map entries, and -- sub-layer right after a full RX chunk -- the chunk's axes in the chunk's record (layer l - 1).
__device__ __forceinline__ void gate_zyz_stores(const GateZ& g, const LayerInfo& prev, int n, int l, int s, int q,
                                                char* __restrict__ rec, char* __restrict__ srec, double* __restrict__ gmap) {
#pragma clang fp contract(off)
    const double2 z = cmul(g.u, g.u);                    // e^{-i alpha}
    double* gm = gmap + ((long)s * n + q) * kGmapDoubles;
    // (everything written here is read by the NEXT launch: write-through stores, nothing left dirty in L2 for the
    // end-of-kernel write-back -- which the next launch waits for)
    store_through(reinterpret_cast<double2*>(gm), make_double2(g.cosb, g.sinb));
    store_through(reinterpret_cast<double2*>(gm) + 1, make_double2(g.cosc, g.sinc));
    store_through(reinterpret_cast<double2*>(gm) + 2, make_double2(z.x, -z.y));
    // Sub-layer right after a full RX chunk: the chunk's gradients are read off THIS sub-layer's inner
    // products (hea_zyz.hpp, bwd_ztri_kernel).  Between the two points lies W = prod_q RY(theta_q) RZ(beta_q),
    // so Im<lam|X_q|psi> there = n . (X, Y, Z)_q here with n the axis of RY RZ X RZ^-1 RY^-1 =
    // (cos beta cos theta, sin beta, -cos beta sin theta)  (the same for wire 4, whose gate runs as RY between
    // RZ(+-pi/2): its Y there is that X).
    // The three numbers ride in the chunk's own record (layer l - 1), whose RY part is otherwise unused.
    if (prev.kind == 0 && prev.m == n && l >= 1) {
        const double2 zb = cmul(g.v, g.v);               // e^{-i beta}
        const double cb = zb.x, sb = -zb.y, ct = g.c * g.c - g.s * g.s, st = 2.0 * g.c * g.s;
        double* em = reinterpret_cast<double*>(rec + (long)(l - 1) * kRecBytes + kRecRy) + 3 * q;
        store_through(em, cb * ct); store_through(em + 1, sb); store_through(em + 2, -cb * st);
        if (srec) {     // ... and in its split record, for the chains that walk back in the split layout (bwd_zquad_kernel)
            double* es = reinterpret_cast<double*>(srec + (long)(l - 1) * kRecBytes + kSRecRy) + 3 * q;
            store_through(es, cb * ct); store_through(es + 1, sb); store_through(es + 2, -cb * st);
        }
    }
}

// The stores of record l by a group of 64 threads (j = index within the group, >= 64: none) from the decompositions of
// layer l's gates (zc: cur is an ansatz sub-layer) and of layer l - 1's (zp: prev is one); zc / zp are not read otherwise.
__device__ __forceinline__ void prep_layer_records(const LayerInfo& cur, const LayerInfo& prev, int n, int l, int j,
                                                   const GateZ* zc, const GateZ* zp,
                                                   char* __restrict__ rec, char* __restrict__ srec) {
#pragma clang fp contract(off)
    char* out = rec + (long)l * kRecBytes;
    if (j < (1 << n)) {
        // products of up to five unit phasors as trees of depth 3 ((f0 f1)(f2 f3)) f4 -- this thread's chain of dependent
        // complex products is the tail of the reduce kernel that writes the next step's records; factors beyond n are 1
        auto tree = [&](const double2 (&zq)[QHEA_MAX_QUBITS], int bits) {
            double2 f[5];
#pragma unroll
            for (int q = 0; q < 5; ++q)
                f[q] = q < n ? (((bits >> q) & 1) ? cconj(zq[q]) : zq[q]) : make_double2(1.0, 0.0);
            return cmul(cmul(cmul(f[0], f[1]), cmul(f[2], f[3])), f[4]);
        };
        double2 ph = make_double2(1.0, 0.0);
        if (cur.kind == 1) {
            double2 vq[QHEA_MAX_QUBITS];
#pragma unroll
            for (int q = 0; q < 5; ++q) vq[q] = zc[q < n ? q : 0].v;
            ph = tree(vq, j);
        }
        if (prev.kind == 1) {
            double2 uq[QHEA_MAX_QUBITS];
#pragma unroll
            for (int q = 0; q < 5; ++q) uq[q] = zp[q < n ? q : 0].u;
            const double2 pu = tree(uq, ring_src_index(n, j));
            ph = cur.kind == 1 ? cmul(ph, pu) : pu;
        }
        // wire 4 of a full RX chunk runs as RZ(-pi/2) RY RZ(pi/2) (hea_zyz.hpp, apply_enc): RZ(pi/2) goes into the
        // diagonal before the chunk, RZ(-pi/2) into the one after it; RZ(phi)|b> = e^{-i phi/2 (1 - 2b)}|b>
        constexpr double kR = 0.70710678118654752440;
        const bool one = (j >> 4) & 1;
        const bool cur_chunk5 = n == 5 && cur.kind == 0 && cur.m == 5, prev_chunk5 = n == 5 && prev.kind == 0 && prev.m == 5;
        if (cur_chunk5) ph = cmul(ph, make_double2(kR, one ? kR : -kR));
        if (prev_chunk5) ph = cmul(ph, make_double2(kR, one ? -kR : kR));
        store_through(reinterpret_cast<double2*>(out) + j, ph);
        if (srec) {     // split records (n = 5, hea_zyz.hpp): wires 0..3 of a full RX chunk run as RZ(-pi/2) RY RZ(pi/2) too
            // four more factors e^{+-i pi/4}, the sign by the wire's bit: together i^k with k = (ones among bits 0..3) - 2 for
            // the chunk of this layer, 2 - ones for the chunk before it -- an exact quarter turn, no multiplication
            const int ones = __popc((unsigned)j & 15u);
            const int k = ((cur_chunk5 ? ones - 2 : 0) + (prev_chunk5 ? 2 - ones : 0)) & 3;
            if (k == 1) ph = make_double2(-ph.y, ph.x);
            else if (k == 2) ph = make_double2(-ph.x, -ph.y);
            else if (k == 3) ph = make_double2(ph.y, -ph.x);
            double* d = reinterpret_cast<double*>(srec + (long)l * kRecBytes + j * 24);
            store_through(d, -ph.y); store_through(d + 1, ph.x); store_through(d + 2, ph.y);
        }
    } else if (j >= 32 && j < 32 + 2 * n) {
        const int q = (j - 32) >> 1, var = (j - 32) & 1;
        if (cur.kind == 1) {    // (an RX chunk's record keeps this part for the next sub-layer's axes, written by ITS block)
            double2 e = make_double2(zc[q].c, var ? zc[q].s : -zc[q].s);
            store_through(reinterpret_cast<double2*>(out + kRecRy + q * 32 + var * 16), e);
            if (srec) {     // (n = 5) wires 0..3: -t / +t; wire 4: the swap form's variants P (c, -s) / P (s, c)
                char* sry = srec + (long)l * kRecBytes + kSRecRy;
                if (q < 4) {
                    const double t = tan_t(zc[q]);
                    store_through(reinterpret_cast<double*>(sry + q * 16 + var * 8), var ? t : -t);
                } else {
                    const double P = tan_scale(zc), pc = P * zc[4].c, ps = P * zc[4].s;
                    store_through(reinterpret_cast<double2*>(sry + 64 + var * 16), var ? make_double2(ps, pc) : make_double2(pc, -ps));
                }
            }
        }
    }
}

// Record of layer l by a group of 64 threads (j = index within the group; threads of the block outside every group pass
// j >= 64 and only join the two barriers).  wfetch(s, k, q) = ansatz angle w[s, k, q] (prep_zyz_kernel: from global memory).
// cur / prev = what layers l and l - 1 are (decode_layer(l < L ? l : -1), decode_layer(l - 1)).  (The reduce kernel that
// writes the next step's records does the first two phases per gate in the lanes of its Adam update instead, and then
// prep_layer_records: the same functions on the same values.)
template <class F>
__device__ __forceinline__ void prep_layer_body(const LayerInfo& cur, const LayerInfo& prev, int n, int l, int j, F wfetch,
                                                char* __restrict__ rec, char* __restrict__ srec, double* __restrict__ gmap,
                                                PrepShared& sh) {
#pragma clang fp contract(off)
    if (j < 0) j = 1 << 30;
    if (j < 6 * n) {
        // (j = which * 3n + k * n + q, without integer divisions)
        const int which = j >= 3 * n, r = j - (which ? 3 * n : 0), k = (r >= n) + (r >= 2 * n), q = r - k * n;
        const LayerInfo& li = which ? prev : cur;
        if (li.kind == 1) {
            double sn, cn;
            fast_sincos(0.5 * wfetch(li.s, k, q), &sn, &cn);
            sh.half[which][k][q] = make_double2(cn, sn);
        }
    }
    __syncthreads();
    if (j < 2 * n) {                                   // one decomposition per thread, then everybody multiplies phasors
        const int which = j >= n, q = j - (which ? n : 0);
        const LayerInfo& li = which ? prev : cur;
        if (li.kind == 1) {
            const GateZ g = gate_zyz(sh.half[which][0][q], sh.half[which][1][q], sh.half[which][2][q]);
            sh.gz[which][q] = g;
            if (which == 0) gate_zyz_stores(g, prev, n, l, li.s, q, rec, srec, gmap);
        }
    }
    __syncthreads();
    prep_layer_records(cur, prev, n, l, j, sh.gz[0], sh.gz[1], rec, srec);
}

// (ensemble launches: member blockIdx.y's angles and workspace slice; the header is slice 0's, whoever the member)
__global__ __launch_bounds__(64) void prep_zyz_kernel(Runs runs, int n, int L, const double* __restrict__ w,
                                                      char* __restrict__ rec, char* __restrict__ srec,
                                                      double* __restrict__ gmap, WorkspaceHeader* hdr, MemberStride ms) {
    const int l = blockIdx.x, j = threadIdx.x;
    const long m = blockIdx.y;
    if (l == 0 && j == 0 && m == 0) header_init(hdr);
    w = member_ptr(w, m * ms.params * (long)sizeof(double));
    rec = member_ptr(rec, m * ms.ws); srec = member_ptr(srec, m * ms.ws); gmap = member_ptr(gmap, m * ms.ws);
    __shared__ PrepShared sh;
    prep_layer_body(decode_layer(runs, n, l < L ? l : -1), decode_layer(runs, n, l - 1), n, l, j,
                    [&](int s, int k, int q) { return w[(long)s * 3 * n + k * n + q]; }, rec, srec, gmap, sh);
}

// Deterministic column sums of a row-major [rows, ncols] matrix: a block owns `cols` consecutive columns
// (cols = max(16, kw), so a sub-layer's X,Y,Z triples never straddle blocks) and splits the rows over
// kRedThreads/cols slices (8 independent loads in flight per thread); partial sums are combined in slice
// order, so results are bitwise reproducible.
constexpr int kRedThreads = 1024;
__host__ __device__ constexpr int red_cols(int kw) { return kw < 16 ? 16 : kw; }

// Rows slice, slice + nslices, ... of TWO adjacent columns (16-byte loads: half the vector-memory instructions of a
// column per thread -- at B = 1024 the sums are bound by the CU's address unit, not by the round trip), each column added in a
// fixed order: eight interleaved accumulators, then a tree.
__device__ __forceinline__ double2 slice_sum2(const double2* __restrict__ p, long rows, long stride_rows2 /* in double2 */,
                                              int slice, int nslices) {
    double2 a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = make_double2(0.0, 0.0);
    long r = slice;
    const long step = (long)nslices * stride_rows2;
    const double2* q = p + (long)slice * stride_rows2;
    for (; r + 7L * nslices < rows; r += 8L * nslices, q += 8 * step) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { const double2 t = q[i * step]; a[i].x += t.x; a[i].y += t.y; }
    }
    // the last (up to seven) rows of the slice: all loads issued together, then added where a row exists -- the same
    // additions as a row-by-row loop, without a memory round trip per row (B = 1024: 256 rows = four per slice, all here)
    double2 t[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) t[i] = (r + (long)i * nslices < rows) ? q[i * step] : make_double2(0.0, 0.0);
#pragma unroll
    for (int i = 0; i < 7; ++i)
        if (r + (long)i * nslices < rows) { a[i].x += t[i].x; a[i].y += t[i].y; }
    return make_double2(((a[0].x + a[1].x) + (a[2].x + a[3].x)) + ((a[4].x + a[5].x) + (a[6].x + a[7].x)),
                        ((a[0].y + a[1].y) + (a[2].y + a[3].y)) + ((a[4].y + a[5].y) + (a[6].y + a[7].y)));
}

// grad_w[s,{0,1,2},q] from the per-wave (X,Y,Z) partial sums (column sums over waves of partial[wave][s][kw]).
//   g_c = Y;  g_b = cos(c) Z + sin(c) X;  g_a = cos(b) Y - sin(b) cos(c) X + sin(b) sin(c) Z
// Returns, in the lanes that own an angle (slice 0, see `tri`), the angle after the update (or as it was: no update); 0 elsewhere.
__device__ __forceinline__ double reduce_xyz_block(int bid, int n, int blk, int kw, long nwaves,
                                                 const double* __restrict__ partial, const double* w /* may alias adam->p */,
                                                 double* __restrict__ grad_w, double* acc /*[kRedThreads]*/, double* stage /*[8 * cols]: LDS apart from acc*/,
                                                 bool poisoned, const double* gmap /* ZYZ-form sums, or nullptr (the fused path rewrites the block's own entries at its end) */,
                                                 const AdamArgs* adam = nullptr, long adam_base = 0,
                                                 int cols_block = 0 /* columns per block if not red_cols(kw) */,
                                                 const DpX* dp = nullptr /* data-parallel step: exchange this block's gradients before the update */,
                                                 int* dp_failed = nullptr /* one int of LDS */,
                                                 double* dp_loc = nullptr /* LDS [kDpBlockValues] */,
                                                 double* dp_xch = nullptr /* LDS [kDpBlockValues * QHEA_DP_MAX_RANKS] */) {
#pragma clang fp contract(off)
    // cols_block = 2 red_cols(kw) (fused path, two sub-layers per block): 64 row slices of 32 columns, so that each column's
    // additions are exactly those of the one-sub-layer blocks (acc then holds 2 kRedThreads values).  Every width here is a
    // power of two (padded_3n): shifts and masks, no integer division in front of the loads.
    const int cols = cols_block ? cols_block : red_cols(kw), nslices = kRedThreads / red_cols(kw);
    const int lc = __builtin_ctz(cols), lk = __builtin_ctz(kw);
    const int tid = (int)threadIdx.x;
    const int j = tid & (cols - 1), slice = tid >> lc;     // roles in the tree and the finish: column j of the block, stage slice
    const int ncols = blk * kw;
    const int v = bid * cols + j;
    // the thread that will finish gate (s, q) fetches what the finish needs first: gradient-map coefficients and the
    // three angles' Adam state travel while the partial rows are being summed
    const int s_fin = v >> lk, r_fin = v & (kw - 1), q_fin = r_fin / 3;
    // Gate (s, q)'s three columns X, Y, Z sit in three adjacent lanes: the X lane (`fin`) turns the sums into the gradients of
    // the gate's three angles, then each of the three lanes (`tri`, role k3) owns ONE angle: its gradient-row entry, its Adam
    // update (three in parallel instead of three in a row), its updated value returned.
    const int k3 = r_fin % 3;
    const bool tri = slice == 0 && v < ncols && r_fin < 3 * n;
    const bool fin = tri && k3 == 0;
    const bool upd = tri && adam && adam->p;
    const long my_idx = adam_base + (long)s_fin * 3 * n + (long)k3 * n + q_fin;     // this lane's angle in the flat vector
    double gmv[6] = {1.0, 0.0, 1.0, 0.0, 1.0, 0.0}, ap = 0.0, am = 0.0, av = 0.0;
    if (fin && gmap) {
        const double* gm = gmap + ((long)s_fin * n + q_fin) * kGmapDoubles;
#pragma unroll
        for (int i = 0; i < 6; ++i) gmv[i] = gm[i];
    }
    if (upd) { ap = adam->p[my_idx]; am = adam->m[my_idx]; av = adam->v[my_idx]; }
    QHEA_STAMP(7);
    {   // sums: thread = (row slice, column PAIR); the threads beyond nslices slices (cols = red_cols(kw): half of them) idle
        const int jp = tid & (cols / 2 - 1), sl = tid >> (lc - 1), vp = bid * cols + 2 * jp;
        if (sl < nslices) {
            double2 r = make_double2(0.0, 0.0);
            if (vp < ncols)
                r = slice_sum2(reinterpret_cast<const double2*>(partial + vp), nwaves, ncols / 2, sl, nslices);
            *reinterpret_cast<double2*>(acc + sl * cols + 2 * jp) = r;
        }
    }
    QHEA_STAMP(8);
    __syncthreads();
    QHEA_STAMP(1);
    // slices are combined in two fixed-order stages (8 interleaved groups, then those 8): a quarter of the serial
    // LDS read chain of a single 64-term loop, and still the same order on every run
    constexpr int kStage = 8;
    // (the first stage's results go to a region of their own and the X lane adds the second stage of its gate's three columns
    // itself -- the same additions in the same order as a thread per column would make: two barriers instead of four)
    // (64 slices, every n <= 5: both stages unrolled, their LDS reads issued together instead of one round trip per term --
    // the additions and their order are those of the loops)
    constexpr int kFull = kStage * kStage;
    double t8 = 0.0;
    if (slice < kStage) {
        if (nslices == kFull) {
            double a[kFull / kStage];
#pragma unroll
            for (int m = 0; m < kFull / kStage; ++m) a[m] = acc[(slice + m * kStage) * cols + j];
#pragma unroll
            for (int m = 0; m < kFull / kStage; ++m) t8 += a[m];
        } else {
            for (int i = slice; i < nslices; i += kStage) t8 += acc[i * cols + j];
        }
        stage[slice * cols + j] = t8;
    }
    __syncthreads();
    QHEA_STAMP(2);
    // the thread that finishes gate (s, q): local gradients of its three angles, then -- data-parallel step -- their sum over
    // the ranks (every thread of the block takes part in the flag / wait phase), then the update
    double gc = 0.0, gb = 0.0, ga = 0.0;
    const int s = s_fin, q = q_fin;
    // second stage: every column's lane adds its own eight values; the X lane then takes Y and Z from its two neighbours
    // (the lanes of slice 0 are all in wave 0: wave shuffles, executed by every wave alike, no barrier)
    double own = 0.0;
    if (tri) {
        if (nslices >= kStage) {
            double a[kStage];
#pragma unroll
            for (int i = 0; i < kStage; ++i) a[i] = stage[i * cols + j];
#pragma unroll
            for (int i = 0; i < kStage; ++i) own += a[i];
        } else {
            for (int i = 0; i < nslices; ++i) own += stage[i * cols + j];
        }
    }
    const double Yn = __shfl_down(own, 1), Zn = __shfl_down(own, 2);
    if (fin) {
        double X = own, Y = Yn;
        const double Z = Zn;
        const double* ws = w + (long)s * 3 * n;
        double sb, cb, sc, cc;
        if (gmap) {     // sums taken after the RY layer, before D_post = RZ(alpha): rotate (X, Y) by alpha (hea_zyz.hpp)
            cb = gmv[0]; sb = gmv[1]; cc = gmv[2]; sc = gmv[3];
            const double ca = gmv[4], sa = gmv[5];
            const double Xr = ca * X - sa * Y;
            Y = ca * Y + sa * X;
            X = Xr;
        } else {
            sincos(ws[n + q], &sb, &cb);
            sincos(ws[2 * n + q], &sc, &cc);
        }
        gc = Y; gb = cc * Z + sc * X; ga = cb * Y - sb * cc * X + sb * sc * Z;
        if (poisoned) gc = gb = ga = std::numeric_limits<double>::quiet_NaN();   // the circuit kernel reported an overrun
    }
    if (dp) {           // (block-uniform)
        // the block's values in flat order: value i = (s - s_first) * 3n + k * n + q  <->  flat element base + i
        const int s_first = (bid * cols) >> lk, s_end = s_first + (cols >> lk) < blk ? s_first + (cols >> lk) : blk;
        const int nvals = (s_end - s_first) * 3 * n, i0 = (s - s_first) * 3 * n + q;
        const long base = adam_base + (long)s_first * 3 * n;
        if (tid == 0) *dp_failed = 0;
        if (fin) { dp_loc[i0] = ga; dp_loc[i0 + n] = gb; dp_loc[i0 + 2 * n] = gc; }
        __syncthreads();
        const bool ok = dpx_exchange_block(*dp, nvals, dp_loc, [base](int i) { return base + i; }, dp_xch, dp_failed);
        if (fin) {
            if (ok) { ga = dpx_sum(*dp, dp_xch, i0); gb = dpx_sum(*dp, dp_xch, i0 + n); gc = dpx_sum(*dp, dp_xch, i0 + 2 * n); }
            else gc = gb = ga = std::numeric_limits<double>::quiet_NaN();
        }
    }
    // the X lane hands gb and gc to its neighbours, and whether any of the three is NaN (some rank's pipeline overran, this
    // rank's, or a failed exchange: no update of the gate anywhere) -- wave shuffles again
    const int bad_x = (ga == ga && gb == gb && gc == gc) ? 0 : 1;
    const double gb_n = __shfl_up(gb, 1), gc_n = __shfl_up(gc, 2);
    const int bad_1 = __shfl_up(bad_x, 1), bad_2 = __shfl_up(bad_x, 2);
    double pn = 0.0;
    if (tri) {
        const double g = k3 == 0 ? ga : k3 == 1 ? gb_n : gc_n;
        const bool skip = poisoned || (k3 == 0 ? bad_x : k3 == 1 ? bad_1 : bad_2) != 0;
        store_through(&grad_w[(long)s * 3 * n + k3 * n + q], g);
        pn = ap;
        if (upd && !skip) pn = adam_update_pre(*adam, my_idx, g, ap, am, av);     // this lane alone reads and writes this angle
    }
    return pn;
}

__global__ __launch_bounds__(kRedThreads) void reduce_kernel(int n, int blk, int kw, long nwaves,
                                                             const double* __restrict__ partial,
                                                             const double* __restrict__ w,
                                                             double* __restrict__ grad_w,
                                                             const WorkspaceHeader* __restrict__ hdr,
                                                             const double* __restrict__ gmap) {
    __shared__ double acc[kRedThreads];
    __shared__ double stage[8 * 64];
    reduce_xyz_block(blockIdx.x, n, blk, kw, nwaves, partial, w, grad_w, acc, stage, hdr->status != 0, gmap);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
int append_blocks(Shape& sh, long count, int enc, int ld) {
    if (count == 0) return QHEA_OK;
    sh.E += count * enc;
    sh.blk += count * ld;
    const int k = sh.runs.nruns;
    if (k > 0 && sh.runs.enc[k - 1] == enc && sh.runs.ld[k - 1] == ld) {
        sh.runs.count[k - 1] += (int)count;
    } else {
        if (k == kMaxRuns) return QHEA_EUNSUPPORTED;
        sh.runs.count[k] = (int)count; sh.runs.enc[k] = enc; sh.runs.ld[k] = ld;
        sh.runs.nruns = k + 1;
    }
    return QHEA_OK;
}

int finish_shape(int n, long nb, Shape& sh) {
    if (sh.E > INT32_MAX || sh.blk > INT32_MAX) return QHEA_EINVAL;
    sh.nblocks = (int)nb;
    sh.fast_ld = zyz_fast_ld(sh.runs, n);
    return QHEA_OK;
}

int make_shape(int n, int nb, const int32_t* enc, const int32_t* ld, Shape& sh) {
    if (n < QHEA_MIN_QUBITS || n > QHEA_MAX_QUBITS || nb < 0) return QHEA_EINVAL;
    if (nb > 0 && (!enc || !ld)) return QHEA_EINVAL;
    sh.runs.nruns = 0;
    for (int b = 0; b < nb; ++b) {
        if (enc[b] < 0 || ld[b] < 0) return QHEA_EINVAL;
        const int rc = append_blocks(sh, 1, enc[b], ld[b]);
        if (rc != QHEA_OK) return rc;
    }
    return finish_shape(n, nb, sh);
}

int simd_count() {                                // of the CURRENT device (cached per device ordinal)
    constexpr int kMaxDev = 64;
    static std::atomic<int> cached[kMaxDev];
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return 1024;
    int v = cached[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) {
            v = 4 * cus;
            cached[dev].store(v, std::memory_order_relaxed);
        } else {
            return 1024;                               // MI355X: 256 CUs x 4 SIMDs (used when no device is visible)
        }
    }
    return v;
}
// BwdArgs::dense (hea_inst.hip: the n = 8, 9 build of bwd_kernel for full devices): the launch has more waves than SIMDs
int dense_bit(long waves) { return waves > simd_count() ? 1 : 0; }

// Backward-kernel choice for n <= 5: QHEA_BWD_AUTO picks by batch density (bwd_kernel_for); the parity tests and the batch
// sweeps force a variant through qhea_set_backward_variant().  Process-wide; it decides the partial-sum layout, so it
// must not change between qhea_workspace_bytes() and the calls that use that size.
std::atomic<int> g_bwd_variant{QHEA_BWD_AUTO};
int use_tri() {                                   // BwdArgs::tri: which first-generation pipelined kernel BwdKernel::PairTri is
    return g_bwd_variant.load(std::memory_order_relaxed) == QHEA_BWD_PAIR ? 0 : 1;   // default: psi / lambda / sigma waves
}

// ---- which kernel a call runs: make_layout (what the workspace holds), then fwd_kernel_for / bwd_kernel_for ----
// What the two kernel rules read besides the call's own traits.  kernel_inputs() fills all of it before make_layout sizes
// anything, from (n, shape, B, Bd, variant, simd_count()): the *_workspace_bytes functions know nothing else.
struct KernelInputs {
    int var, simd;              // the variant and simd_count() the layout was made under
    bool lds;                   // n >= 10: workgroup-resident kernels
    bool records;               // a ZYZ-eligible shape under a variant that runs the ZYZ kernels
    bool srecords;              // ... n = 5, block-unrolled shape, table fits: forward sweeps and chains in the split layout
    bool fast;                  // records, and the shape is block-unrolled
    bool two_fit;               // two pipelines' LDS (bwd_ztri_kernel<N, 2>) fits a workgroup
    bool single;                // B == Bd: not a launch of several members
    long rows_d, groups_d, fwd_waves_d;     // rows, sample groups and forward waves of the LAUNCH (Bd)
};
// What sizes the workspace, and so must agree between the *_workspace_bytes functions and the calls.
struct Layout {
    KernelInputs in;            // what fwd_kernel_for / bwd_kernel_for take
    size_t off_U, off_cs, off_part, off_rec, off_srec, off_gmap, off_snap, total;
    long nwaves, nwaves_fwd;    // partial rows of the backward kernel; waves of the first-generation / private-ring forward
    int zL;                     // ZYZ layer count (records 0 .. zL)
    bool records, srecords;     // layer records and gmap / split records exist (in.records, in.srecords)
    bool snaps;                 // psi snapshots of the forward sweep at off_snap: the layouts whose backward is bwd_zsnap_kernel
    // "Is the backward of the ZYZ family" (prep_zyz_kernel, sums through gmap), for every caller that asks it: the same as
    // zyz_family(bwd_kernel_for(in, n, traits)) under ANY traits, because bwd_kernel_for reads the traits only to choose
    // between ZYZ kernels (ZSnap / ZTri2, ZQuad / ZTri1).  The forward's family is another question: zyz_family(fwd_kernel_for).
    bool zyz_bwd;
};

// The kernels that exist.  The ZYZ family (hea_zyz.hpp, n <= 5) comes last in both.
enum class FwdKernel { First /* fwd_kernel */, Lds /* lds_fwd_kernel */, Zyz /* fwd_zyz_kernel: a record ring per wave */,
                       ZShared /* fwd_zshared_kernel: one ring per workgroup */, Split /* fwd_split_kernel */ };
enum class BwdKernel { Packed /* bwd_kernel, dense or not: dense_bit */, PairTri /* bwd_pair_kernel / bwd_tri_kernel: use_tri */,
                       Lds /* lds_bwd_kernel */, ZTri1, ZTri2 /* bwd_ztri_kernel<N, 1 / 2> */, ZPacked, ZQuad, ZSnap };
inline bool zyz_family(FwdKernel k) { return k >= FwdKernel::Zyz; }
inline bool zyz_family(BwdKernel k) { return k >= BwdKernel::ZTri1; }
// what a call adds to its layout: the read-out, whether the backward is given the final state, members in the launch
struct CallTraits { int pauli = QHEA_PAULI_Z; bool state_given = false; int R = 1; };

FwdKernel fwd_kernel_for(const KernelInputs& in, const CallTraits& c) {
    // Workgroup-resident kernels (hea_lds.hip) for n >= 10; the wave-resident ones are built for n <= 9 only.
    // Measured when both existed, 12 sub-layers, B = 1024, forward / forward+backward:
    //   n = 10: 67 / 232 us vs 97 / 263 us wave-resident;  n = 11: 110 / 450 vs 144 / 1250 us (the wave-resident
    //   backward spills);  n = 12: 205 / 880 us vs 367 us / 12.4 ms.
    if (in.lds) return FwdKernel::Lds;
    // second-generation kernels for n <= 5 (hea_zyz.hpp): the default when the shape is eligible (in.records); the
    // first-generation forward takes over for shapes whose (cos, sin) table exceeds LDS.
    // Measured at cfg 2's circuit (us per call incl. prep; first-generation / ZYZ form):
    //   forward   B = 1024 55 / 44,  4096 87 / 89,  16384 236 / 255 with a record ring per wave (22 KB of LDS per wave
    //             cap the waves per CU once the batch could fill them) -> one ring per workgroup beyond one wave per SIMD
    // so: private-ring kernel while the sweeps leave SIMDs free, shared-ring kernel (block-unrolled shapes) beyond;
    // other shapes fall back to the first-generation forward once two waves per SIMD are reached
    const int var = in.var;
    const bool shared = in.fast && (var == QHEA_BWD_ZPACKED || (var == QHEA_BWD_AUTO && in.fwd_waves_d > (long)in.simd));
    const bool zyz = in.records && (shared || var == QHEA_BWD_ZTRI || var == QHEA_BWD_ZTRI2 || var == QHEA_BWD_ZQUAD ||
                                   var == QHEA_BWD_ZSNAP || in.fwd_waves_d <= 2L * in.simd);
    if (!zyz) return FwdKernel::First;
    if (shared) return FwdKernel::ZShared;
    // split forward, one sample per wave: pays while every sweeping wave still gets a SIMD of its own; Z / diagonal read-out
    // only -- X or Y: the private-ring forward
    if (in.srecords && in.rows_d <= (int64_t)in.simd && c.pauli == QHEA_PAULI_Z) return FwdKernel::Split;
    return FwdKernel::Zyz;
}

BwdKernel bwd_kernel_for(const KernelInputs& in, int n, const CallTraits& c) {
    if (in.lds) return BwdKernel::Lds;                  // n >= 10 (measurements: fwd_kernel_for)
    const int var = in.var;
    const long cus = (long)in.simd / 4;
    // Pipelined backward kernels (n <= 5): several waves per sample group (psi chain, lambda chain, sigma waves), so they
    // pay while the packed kernel would leave SIMDs without a wave (hea_device.hpp: bwd_tri_kernel, bwd_pair_kernel).
    // Measured at n = 5, cfg 2's circuit (us per training step, pipelined in two rounds / one wave per group,
    // profiles/r03_batch_sweep.txt, end of round 3): B = 1100 141.3 / 153.3, 1280 142.0 / 154.3, 1536 144.2 / 155.8,
    // 1792 216.2 / 156.9 -- pipelined while the sample groups fill at most 6/8 of the SIMDs (3 per CU: two rounds of the
    // one-pipeline workgroups; the third round starts beyond)
    const bool pipelined = n <= 5 && in.rows_d > 0 && var != QHEA_BWD_PACKED && var != QHEA_BWD_ZPACKED &&
                           (var != QHEA_BWD_AUTO || 8 * in.groups_d <= 6 * (int64_t)in.simd);
    // Measured at cfg 2's circuit (us per call incl. prep / reduce):
    //   backward  B = 1024 packed 189, tri 135, ztri 115, zpacked 173;  2048 251 / 255 / 208 / 180;
    //             4096 302 / 400 / 402 / 258;  16384 1159 / 1405 / 1580 / 846   (scripts/ablate/bsweep_all.py)
    // so AUTO keeps round 1's rule for the pipeline (sample groups on at most 3/4 of the SIMDs) and, for batches that fill the
    // SIMDs, takes the one-wave ZYZ kernel for the block-unrolled shapes (B = 16384 at cfg 2's circuit: see DESIGN.md section
    // 3.5), the first-generation packed kernel otherwise
    if (in.fast && (var == QHEA_BWD_ZPACKED || (var == QHEA_BWD_AUTO && !pipelined))) return BwdKernel::ZPacked;
    if (!pipelined) return BwdKernel::Packed;
    // the first-generation pipeline stays selectable (QHEA_BWD_PAIR / TRI) and takes over for shapes whose (cos, sin) table
    // exceeds LDS
    if (!in.records) return BwdKernel::PairTri;
    // Two pipelines per workgroup (bwd_ztri_kernel<N, 2>: their sigma waves add the two groups' sums in LDS, half the partial
    // rows).  With the chain waves laid out as the workgroup's waves 0..3 every SIMD hosts exactly ONE of the CU's four chain
    // waves; two separate five-wave workgroups (and round 2's pipeline-by-pipeline layout of the ten) put two chains on one
    // SIMD, and the pipeline runs at the pace of its slowest chain.  cfg 2, us per training step, two pipelines per workgroup /
    // one: B = 520 89.5 / 96.1, 640 90.0 / 97.8, 768 90.6 / 98.5, 896 91.1 / 99.3, 1024 91.3 / 101.1 (profiles/r03_batch_sweep.txt)
    // -- so AUTO takes two pipelines wherever the batch has more sample groups than the device has CUs (up to two per CU; beyond
    // that the one-pipeline workgroups run in two rounds, 154 us at 1280).  QHEA_BWD_ZTRI2 forces them, QHEA_BWD_ZTRI never.
    const bool auto_two = var == QHEA_BWD_AUTO && in.groups_d > cus && in.groups_d <= 2 * cus;
    const bool two_wanted = var == QHEA_BWD_ZTRI2 ? in.groups_d > cus : (var == QHEA_BWD_ZSNAP || auto_two);
    if (two_wanted && in.two_fit) {
        // Snapshot pipeline (bwd_zsnap_kernel): where AUTO takes two pipelines per workgroup, the sigma waves read psi from the
        // forward sweep's snapshots instead of a psi chain walking back (cfg 2, B = 1024: kernel 74.5 -> 70.0 us, step 0.0828 ->
        // 0.0783 ms).  Single-model layouts only (ensembles keep bwd_ztri_kernel); X or Y read-out, a
        // given final state or several members: the two-pipeline ztri kernel
        const bool snap_wanted = var == QHEA_BWD_ZSNAP || auto_two;
        if (in.srecords && in.single && snap_wanted && n == 5 && c.pauli == QHEA_PAULI_Z && !c.state_given && c.R == 1)
            return BwdKernel::ZSnap;
        return BwdKernel::ZTri2;
    }
    // Quad-chain pipeline: where every CU holds at most one sample group the step time is the length of the dependent chain,
    // and the split-layout reverse walk shortens it (cfg 2's circuit, us per training step, all-lane / split reverse walk:
    // DESIGN.md section 3.3a).  Same partial-row layout as the one-pipeline kernel, which X or Y read-outs fall back to.
    const bool quad_wanted = var == QHEA_BWD_ZQUAD || (var == QHEA_BWD_AUTO && in.groups_d <= cus);
    if (in.srecords && quad_wanted && n == 5 && c.pauli == QHEA_PAULI_Z) return BwdKernel::ZQuad;
    return BwdKernel::ZTri1;
}

// B: rows of ONE model, which sizes the workspace (partial rows, tables); Bd: rows the launch carries, which choose the kernels
// -- R x B for an ensemble launch of R members (qhea_model_ensemble_train_steps: the occupancy rules above are about the whole
// grid), B otherwise.
KernelInputs kernel_inputs(int n, const Shape& sh, int64_t B, int64_t Bd) {
    KernelInputs in{};
    const int spw = 64 >> lane_bits(n);                // samples per wave of the wave-resident kernels
    const int var = g_bwd_variant.load(std::memory_order_relaxed);
    in.var = var; in.simd = simd_count(); in.lds = lds_supported(n);
    in.records = zyz_eligible(n, sh.E) &&
                 (var == QHEA_BWD_AUTO || var == QHEA_BWD_ZTRI || var == QHEA_BWD_ZTRI2 || var == QHEA_BWD_ZPACKED ||
                  var == QHEA_BWD_ZQUAD || var == QHEA_BWD_ZSNAP);
    in.fast = in.records && sh.fast_ld != 0;
    in.srecords = in.records && zsplit_eligible(n, sh.E, sh.runs);
    in.two_fit = in.records && 2 * ztri_fixed_lds(kZRingDepth<2>) + 2 * (size_t)(64 >> n) * zyz_cs_row(n, sh.E) * (in.srecords ? 32 : 16) +
                                   (size_t)sh.blk * padded_3n(n) * sizeof(double) <= 158 * 1024;
    in.single = B == Bd; in.rows_d = Bd;
    in.groups_d = (Bd + spw - 1) / spw;
    in.fwd_waves_d = ((in.groups_d + kWaves - 1) / kWaves) * kWaves;
    return in;
}
Layout make_layout(int n, const Shape& sh, int64_t B, int64_t Bd) {
    Layout L{};
    const int spw = 64 >> lane_bits(n);
    auto round_waves = [](long w) { return ((w + kWaves - 1) / kWaves) * kWaves; };   // padding waves write zeros
    L.in = kernel_inputs(n, sh, B, Bd);
    L.records = L.in.records; L.srecords = L.in.srecords;
    L.zL = L.records ? zyz_layer_count(sh.runs, n) : 0;
    // the backward family first (the fall-backs by read-out, given state or member count stay inside a family's partial-row
    // layout), then the partial rows from it
    const BwdKernel fam = bwd_kernel_for(L.in, n, CallTraits{});
    L.zyz_bwd = zyz_family(fam);
    L.snaps = fam == BwdKernel::ZSnap;
    const long groups = (B + spw - 1) / spw;
    L.nwaves_fwd = round_waves(groups);
    switch (fam) {
        case BwdKernel::Lds:     L.nwaves = B; break;                                      // one row per sample
        case BwdKernel::Packed:  L.nwaves = round_waves(groups); break;
        case BwdKernel::ZPacked: L.nwaves = (groups + kZPWaves - 1) / kZPWaves; break;     // one row per WORKGROUP (its four waves' sums added in LDS)
        case BwdKernel::ZTri2: case BwdKernel::ZSnap: L.nwaves = (groups + 1) / 2; break;  // one row per workgroup = two sample groups
        default:                 L.nwaves = groups; break;                                 // one row per workgroup = sample group
    }
    const TableLayout t = table_layout(n, sh, B);
    L.off_U = t.off_gates; L.off_cs = t.off_cs;
    size_t p = t.end;
    L.off_part = p; p = align256(p + (size_t)L.nwaves * sh.blk * padded_3n(n) * sizeof(double));
    const size_t rec_bytes = (size_t)(L.zL + 1 + 2 * kPadRecs) * kRecBytes;                       // padded both sides
    L.off_rec = p;  p = align256(p + (L.records ? rec_bytes : 0));
    if (L.records) L.off_rec += (size_t)kPadRecs * kRecBytes;                                     // -> record 0
    L.off_srec = p; p = align256(p + (L.srecords ? rec_bytes : 0));
    if (L.srecords) L.off_srec += (size_t)kPadRecs * kRecBytes;
    L.off_gmap = p; p = align256(p + (L.records ? (size_t)sh.blk * n * kGmapDoubles * sizeof(double) : 0));
    // psi of every sample group at every publication point, 1 KB each (61 MB at B = 1024, cfg 2); the region exists only in the
    // layouts that select the snapshot kernel, so qhea_workspace_bytes agrees with the call
    L.off_snap = p;
    if (L.snaps) p = align256(p + (size_t)(2 * L.nwaves) * sh.nblocks * sh.fast_ld * kSnapBytes);
    L.total = p;
    return L;
}
Layout make_layout(int n, const Shape& sh, int64_t B) { return make_layout(n, sh, B, B); }

__global__ void adam_kernel(long n, const double* __restrict__ g, AdamArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) adam_update(a, i, g[i]);
}

thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;
inline void profile_begin(hipStream_t st) { if (g_ev_start) (void)hipEventRecord(g_ev_start, st); }
inline void profile_end(hipStream_t st) {
    if (g_ev_stop) (void)hipEventRecord(g_ev_stop, st);
    g_ev_start = nullptr; g_ev_stop = nullptr;
}

// R, ms: an ensemble launch (member = blockIdx.y, hea_zyz.hpp: MemberStride); ws and w are member 0's
int launch_prep_zyz(int n, const Shape& sh, const double* w, char* ws, const Layout& L, hipStream_t st, int R = 1,
                    const MemberStride& ms = MemberStride{}) {
    hipLaunchKernelGGL(prep_zyz_kernel, dim3((unsigned)(L.zL + 1), (unsigned)R), dim3(64), 0, st, sh.runs, n, L.zL, w,
                       ws + L.off_rec, L.srecords ? ws + L.off_srec : nullptr, reinterpret_cast<double*>(ws + L.off_gmap),
                       reinterpret_cast<WorkspaceHeader*>(ws), ms);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}
// The ZYZ-family forward kernel k (fwd_kernel_for): its grid, its LDS bytes, its launch.  Like every circuit-kernel launcher
// here, timed by qhea_profile_next_circuit_kernel; QHEA_EUNSUPPORTED: a qubit count this build lacks
int launch_zyz_forward(FwdKernel k, int n, const Shape& sh, int64_t B, const Layout& L, char* ws, const AngleSrc& src, double off,
                       double co, const double* diag, int pauli, double* out, double* state_out, const double* bias,
                       hipStream_t st) {
    const ZFwdArgs za{sh.runs, (long)B, (int)sh.E, ws + L.off_rec, (int)((L.zL + 1) * kRecBytes), L.zL, src, off, co, diag,
                      pauli, out, state_out, bias, sh.fast_ld, sh.nblocks, L.srecords ? ws + L.off_srec : nullptr};
    const size_t group_cs = (size_t)(64 >> n) * zyz_cs_row(n, sh.E) * sizeof(double2);    // a sample group's (cos, sin) table
    const long groups = (B + (64 >> n) - 1) / (64 >> n);
    const dim3 shared_grid((unsigned)((groups + kZPWaves - 1) / kZPWaves));
    const dim3 ring_grid((unsigned)((L.nwaves_fwd + kZFwdWaves - 1) / kZFwdWaves));
    int rc = QHEA_EUNSUPPORTED;
    profile_begin(st);
    if (k == FwdKernel::Split) {
        launch_fwd_split_5(dim3((unsigned)((B + kSplitWaves - 1) / kSplitWaves)), (size_t)kSplitWaves * zyz_cs_row(5, sh.E) * 32, st, za);
        rc = QHEA_OK;
    } else if (k == FwdKernel::ZShared) switch (n) {
#define QHEA_CASE(NN) case NN: launch_fwd_zshared_##NN(shared_grid, kZPWaves * group_cs, st, za); rc = QHEA_OK; break;
        QHEA_FOR_EACH_ZN(QHEA_CASE)
#undef QHEA_CASE
    } else if (k == FwdKernel::Zyz) switch (n) {
#define QHEA_CASE(NN) case NN: launch_fwd_zyz_##NN(ring_grid, kZFwdWaves * group_cs, st, za); rc = QHEA_OK; break;
        QHEA_FOR_EACH_ZN(QHEA_CASE)
#undef QHEA_CASE
    }
    profile_end(st);
    if (rc != QHEA_OK) return rc;
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}
// the ZYZ-family backward kernel k (bwd_kernel_for): one partial row per workgroup, member = blockIdx.y
int launch_zyz_backward(BwdKernel k, int n, const Shape& sh, int64_t B, const Layout& L, char* ws, const AngleSrc& src, double off,
                        double co, const double* diag, int pauli, const double* g, const double* state_in, const double* y,
                        const double* bias, double inv_bt, double* out, double* grad_x, double* partial, hipStream_t st,
                        int R = 1, const MemberStride& ms = MemberStride{}, const char* mrec = nullptr) {
    const int pipes = (k == BwdKernel::ZTri2 || k == BwdKernel::ZSnap) ? 2 : 1;
    const bool split = L.srecords && k != BwdKernel::ZPacked;       // the chains sweep forward in the split layout
    ZBwdArgs za{sh.runs, (long)B, (int)sh.E, (int)sh.blk, ws + L.off_rec, (int)((L.zL + 1) * kRecBytes), L.zL, src, off, co,
                      diag, pauli, g, state_in, y, bias, inv_bt, out, grad_x, partial,
                      &reinterpret_cast<WorkspaceHeader*>(ws)->status, sh.fast_ld, sh.nblocks,
                      split ? ws + L.off_srec : nullptr, pipes};
    za.ms = ms;
    za.src.m_rows = ms.rows; za.src.m_params = ms.params;
    const dim3 grid((unsigned)L.nwaves, (unsigned)R);
    const size_t dyn = (size_t)(64 >> n) * zyz_cs_row(n, sh.E) * sizeof(double2);
    const size_t sums = (size_t)sh.blk * padded_3n(n) * sizeof(double);      // two pipelines: their sums added in LDS
    const size_t dyn_tri = (size_t)pipes * (ztri_fixed_lds(pipes == 2 ? kZRingDepth<2> : kZRingDepth<1>) + (split ? 2 * dyn : dyn)) +
                           (pipes == 2 ? sums : 0);
    int rc = QHEA_EUNSUPPORTED;
    profile_begin(st);
    if (k == BwdKernel::ZSnap) {
        za.snap = ws + L.off_snap;
        launch_bwd_zsnap_5(grid, 2 * (zsnap_fixed_lds(kZSnapRing) + 2 * dyn) + sums, st, za);
        rc = QHEA_OK;
    } else if (k == BwdKernel::ZQuad) {
        launch_bwd_zquad_5(grid, zquad_fixed_lds(kPairRing) + 2 * dyn, st, za, mrec);
        rc = QHEA_OK;
    } else if (k == BwdKernel::ZPacked) switch (n) {
#define QHEA_CASE(NN) case NN: launch_bwd_zpacked_##NN(grid, zp_cs_bytes(n, sh.E, kZPWaves * (64 >> n)), st, za, mrec); rc = QHEA_OK; break;
        QHEA_FOR_EACH_ZN(QHEA_CASE)
#undef QHEA_CASE
    } else if (k == BwdKernel::ZTri1 || k == BwdKernel::ZTri2) switch (n) {
#define QHEA_CASE(NN) case NN: launch_bwd_ztri_##NN(grid, dyn_tri, st, za, mrec); rc = QHEA_OK; break;
        QHEA_FOR_EACH_ZN(QHEA_CASE)
#undef QHEA_CASE
    }
    profile_end(st);
    if (rc != QHEA_OK) return rc;
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

// The first-generation and workgroup-resident circuit kernels (FwdKernel::First / Lds, BwdKernel::Packed / PairTri / Lds) on the
// tables of prep_kernel / prep_model_kernel
int launch_table_forward(FwdKernel k, int n, const Shape& sh, int64_t B, const Layout& L, const char* ws, double off, double co,
                         const double* diag, int pauli, double* out, double* state_out, const double* bias, hipStream_t st) {
    const FwdArgs fa{sh.runs, (long)B, (int)sh.E, reinterpret_cast<const double2*>(ws + L.off_cs), ws + L.off_U,
                     (int)((sh.blk + 2) * n * kGateBytes), off, co, diag, out, state_out, bias, pauli};
    const dim3 grid((unsigned)(L.nwaves_fwd / kWaves));
    profile_begin(st);
    if (k == FwdKernel::Lds) {
        if (launch_lds_fwd(n, (long)B, st, fa) != QHEA_OK) return QHEA_ELAUNCH;
    } else switch (n) {
#define QHEA_CASE(NN) case NN: launch_fwd_##NN(grid, st, fa); break;
        QHEA_FOR_EACH_N(QHEA_CASE)
#undef QHEA_CASE
        default: return QHEA_EUNSUPPORTED;
    }
    profile_end(st);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}
int launch_table_backward(BwdKernel k, int n, const Shape& sh, int64_t B, const Layout& L, char* ws, double off, double co,
                          const double* diag, int pauli, const double* g, const double* state_in, const double* y,
                          const double* bias, double inv_bt, double* out, double* grad_x, double* partial, hipStream_t st) {
    const BwdArgs ba{sh.runs, (long)B, (int)sh.E, (int)sh.blk, reinterpret_cast<const double2*>(ws + L.off_cs), ws + L.off_U,
                     (int)((sh.blk + 2) * n * kGateBytes), off, co, diag, g, state_in, y, bias, inv_bt, out, grad_x, partial,
                     pauli, use_tri(), dense_bit(L.nwaves), &reinterpret_cast<WorkspaceHeader*>(ws)->status};
    const dim3 packed_grid((unsigned)(L.nwaves / kWaves)), group_grid((unsigned)L.nwaves);
    profile_begin(st);
    if (k == BwdKernel::Lds) {
        if (launch_lds_bwd(n, (long)B, st, ba) != QHEA_OK) return QHEA_ELAUNCH;
    } else switch (n) {
#define QHEA_CASE(NN) case NN: if (k == BwdKernel::PairTri) launch_bwd_pair_##NN(group_grid, st, ba); else launch_bwd_##NN(packed_grid, st, ba); break;
        QHEA_FOR_EACH_N(QHEA_CASE)
#undef QHEA_CASE
        default: return QHEA_EUNSUPPORTED;
    }
    profile_end(st);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

int launch_prep(int n, const Shape& sh, int64_t B, const double* w, const double* x, char* ws, const Layout& L,
                hipStream_t st) {
    const long total = (sh.blk + 2) * n + B * sh.E;
    const int threads = 256;
    const long blocks = (total + threads - 1) / threads;
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, n, (int)sh.blk, w,
                       reinterpret_cast<double4*>(ws + L.off_U), (long)(B * sh.E), x,
                       reinterpret_cast<double2*>(ws + L.off_cs), reinterpret_cast<WorkspaceHeader*>(ws));
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}


// ---------------------------------------------------------------------------------------
// model-level (fused) path: frequency layers + sincos in prep, MSE residual in the circuit
// kernel, every parameter gradient in one reduce launch
// ---------------------------------------------------------------------------------------
// gate-table entry tid (n padding entries on each side) of the model-level prep kernels
__device__ __forceinline__ void prep_gate_entry(int n, int blk, const double* __restrict__ w, double4* __restrict__ gates, long tid) {
    const long g = tid - n;
    double4 v0 = make_double4(1.0, 0.0, 0.0, 0.0);
    if (g >= 0 && g < (long)blk * n) {
        const int s = (int)(g / n), q = (int)(g % n);
        const double* ws = w + (long)s * 3 * n;
        double sa, ca, sb, cb, sc, cc;
        fast_sincos(0.5 * ws[q], &sa, &ca);
        fast_sincos(0.5 * ws[n + q], &sb, &cb);
        fast_sincos(0.5 * ws[2 * n + q], &sc, &cc);
        const double m00r = cb * ca, m00i = -sb * ca, m01r = -cb * sa, m01i = sb * sa;
        const double m10r = cb * sa, m10i = sb * sa, m11r = cb * ca, m11i = sb * ca;
        v0 = make_double4(cc * m00r - sc * m10r, cc * m00i - sc * m10i,
                          cc * m01r - sc * m11r, cc * m01i - sc * m11i);
    }
    gates[2 * tid] = v0;
    gates[2 * tid + 1] = make_double4(v0.x, -v0.y, -v0.z, v0.w);
}
__global__ void prep_model_kernel(int n, int blk, const double* __restrict__ w, double4* __restrict__ gates,
                                  long B, int E, EncDesc enc, double2* __restrict__ cs, WorkspaceHeader* hdr) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid == 0) header_init(hdr);
    const long ng = (long)(blk + 2) * n;
    if (tid < ng) {
        prep_gate_entry(n, blk, w, gates, tid);
    } else if (tid - ng < B * E) {
        const long t = tid - ng;
        const long b = t / E;
        int e = (int)(t % E);
        const int si = e < enc.seg[0].ncols ? 0 : 1;
        const EncSeg& sg = enc.seg[si];
        if (si) e -= enc.seg[0].ncols;
        const double v = sg.in[b * sg.width + e % sg.width];
        const double x = sg.w ? v * sg.w[e] + sg.b[e] : v * sg.scale;
        double s, c;
        fast_sincos(0.5 * x, &s, &c);
        cs[t] = make_double2(c, s);
    }
}

struct GradMap {                // where each gradient lives in the flat output
    long off_ans, off_bias, off_sse;         // off_bias < 0: model has no bias
    long off_w[2], off_b[2];                 // per encoding segment; < 0: not trainable
};

// Roles by block index: [0, nb_w) ansatz gradients from the (X,Y,Z) partials; [nb_w, nb_w+nb_x)
// frequency-layer gradients from grad_x (16 columns x 64 row slices per block); last block: bias gradient,
// sse, sum y^2.
// (8 columns = 64 B per row: a frequency block is bound by what ONE CU can pull -- its columns of grad_x and of the inputs over
// all B rows -- and it was the reduce kernel's longest block at 16 columns once the ansatz blocks' records got cheaper)
constexpr int kFreqCols = 8, kFreqSlices = kRedThreads / kFreqCols, kFreqStage = 8;
// Records of the NEXT training step written by this one's reduce kernel (qhea_model_train_steps, block-unrolled shapes:
// every block = one full RX chunk + ld sub-layers).  One reduce block then owns a whole circuit block -- ld x kw columns,
// its ld sub-layers' angles and Adam state -- and, once it has updated them, three 64-thread groups write the records that
// depend on nothing else: the block's ld sub-layers' and the FOLLOWING chunk's (or the final record's), whose diagonals
// take this block's last sub-layer through the ring.  The first chunk's record never changes.  No prep launch then.
struct FusePrep {
    int nbk;                // circuit blocks per reduce block: 1, or 2 where a block's columns fill half a reduce block (n = 2, ld = 1)
    int ld;                 // 0: off
    int L;                  // layer count (records 0 .. L)
    Runs runs;
    char* rec; char* srec; double* gmap;
};
constexpr int kFuseMaxLd = 2;
// DP (the data-parallel step, qhea_model_dp_train_steps): every block publishes the LOCAL gradients it has just formed to
// the peers' exchange buffers, waits for the peers' (flags per block), adds them in rank order and only then writes the
// gradient row, updates and -- FUSE -- writes the next records: the sum over the ranks costs no launch of its own
// (hea_dp.hpp; bitwise the results of qhea_model_loss_grad + qhea_dp_allreduce_adam).
// Member learning rates (MT, ensemble launches of R > 1 members): member blockIdx.y's Adam step size is its MemberRec::lr
// divided by the step's bias correction 1 - beta1^t, here, in IEEE double division -- the same rounding as the host's lr / bc1
// of a single-model call.  The member's other Adam arguments are the launch's.
struct MemberLr {
    const char* mrec;           // member 0's MemberRec (hea_zyz.hpp), member m's ms.ws bytes further per member
    double bc1;
};
// Depth sweeps (DEPTH, with MT; qhea_model_depth_sweep_train_steps): member blockIdx.y's block counts are its MemberRec::depth,
// and its blk, E, parameter layout and block roles follow from them (depth_map).  The launch's blk, E, gm.off_ans / off_sse /
// off_w / off_b, nb_w and nb_x are the largest member's and not used; w is the member's parameter row (not its angles).  The
// grid is sized for the largest member: a block beyond its member's last role returns at once.
struct DepthMap {
    int blk, E, nc0;                        // sub-layers, encoding columns, columns of segment 0
    long off_w0, off_b0, off_w1, off_b1;    // frequency weights / biases per segment (< 0: fixed frequency)
    long off_ans, P;
};
__host__ __device__ inline DepthMap depth_map(int n, bool quanonet, bool trainable, int c0, int c1, int ld0, int ld1) {
    DepthMap d;                             // (the layout of model_info: bias, branch_freq, trunk_freq, quantum_layer)
    d.nc0 = c0 * n;
    const int nc1 = c1 * n;
    d.E = d.nc0 + nc1;
    d.blk = c0 * ld0 + c1 * ld1;
    d.off_w0 = d.off_b0 = d.off_w1 = d.off_b1 = -1;
    long p = quanonet ? 1 : 0;
    if (trainable) {
        if (quanonet) { d.off_w1 = p; p += nc1; d.off_b1 = p; p += nc1; }
        d.off_w0 = p; p += d.nc0; d.off_b0 = p; p += d.nc0;
    }
    d.off_ans = p;
    d.P = p + (long)d.blk * 3 * n;
    return d;
}
struct DepthRed { int quanonet, trainable, ld0, ld1; };
// Qubit sweeps (QS, a DEPTH form; qhea_model_qubit_sweep_train_steps): the members differ in n as well.  The grid is a flat
// list of every member's own roles -- work-list entries (member, role) in the slices' list regions (hea_qsweep.hpp: QsWork) --
// and the member's n is its MemberRec::nq; its kw and partial-row count follow from it and the batch.  The launch's n, kw and
// nwaves are not used.
struct QubitRed {
    DepthRed dr;
    QsWork wk;
};
__device__ __forceinline__ DepthRed dr_of(const DepthRed& d) { return d; }
__device__ __forceinline__ DepthRed dr_of(const QubitRed& q) { return q.dr; }
// DR: empty, one DepthRed (the depth-sweep instantiation) or one QubitRed (the qubit-sweep one); the others keep their exact
// argument list
template <bool FUSE, bool DP, bool MT = false, class... DR>   // (the fused one's LDS and registers do not weigh on the plain one)
__global__ __launch_bounds__(kRedThreads) void reduce_model_kernel(
        int n, int blk, int kw, long nwaves, const double* __restrict__ partial, const double* w,
        long B, int E, EncDesc enc, const double* __restrict__ grad_x, const double* __restrict__ pred,
        const double* __restrict__ y, double inv_bt, GradMap gm, int nb_w, int nb_x, double* __restrict__ grad,
        AdamArgs adam, const WorkspaceHeader* __restrict__ hdr, const double* gmap, FusePrep fp, DpX dpx, MemberStride ms,
        MemberLr mlr, DR... dr_pack) {
#pragma clang fp contract(off)
    constexpr bool DEPTH = sizeof...(DR) != 0;
    constexpr bool QS = (std::is_same<DR, QubitRed>::value || ...);
    static_assert(!DEPTH || (MT && !FUSE && !DP), "depth sweeps: member learning rates, no fused records, one rank");
    // A depth-sweep member's own GradMap entries and segment-0 width: locals (a modified copy of gm or enc would live in private
    // memory); the other instantiations read the arguments where they are used, as they always did
    long d_ans = 0, d_sse = 0, d_w0 = 0, d_b0 = 0, d_w1 = 0, d_b1 = 0;
    int d_nc0 = 0;
    auto g_ans = [&]() -> long { if constexpr (DEPTH) return d_ans; else return gm.off_ans; };
    auto g_sse = [&]() -> long { if constexpr (DEPTH) return d_sse; else return gm.off_sse; };
    auto nc0 = [&]() -> int { if constexpr (DEPTH) return d_nc0; else return enc.seg[0].ncols; };
    long mem = blockIdx.y;                              // member and role of this block (QS: its work-list entry's)
    int bid = blockIdx.x;
    if constexpr (QS) {
        const int2 ent = qs_entry((dr_pack, ...).wk, ms.ws, (int)blockIdx.x);
        mem = ent.x; bid = ent.y;
    }
    {   // ensemble launches: member blockIdx.y's data, parameters, gradient rows and workspace slice (hdr: slice 0's)
        const long m = mem, wsb = m * ms.ws, pb = m * ms.params * (long)sizeof(double);
        if constexpr (MT) {
            const MemberRec* mr = member_ptr(reinterpret_cast<const MemberRec*>(mlr.mrec), wsb);
            adam.lr_over_bc1 = ((ConstMemberRec)mr)->lr / mlr.bc1;
            if constexpr (QS) {                         // the member's own qubit count
                n = ((ConstMemberRec)mr)->nq;
                kw = padded_3n(n);
                nwaves = qs_part_rows(n, B);
            }
            if constexpr (DEPTH) {
                const DepthRed dr = dr_of((dr_pack, ...));
                const DepthMap d = depth_map(n, dr.quanonet != 0, dr.trainable != 0, ((ConstMemberRec)mr)->depth[0],
                                             ((ConstMemberRec)mr)->depth[1], dr.ld0, dr.ld1);
                blk = d.blk; E = d.E; d_nc0 = d.nc0;
                nb_w = (blk * kw + red_cols(kw) - 1) / red_cols(kw);
                nb_x = dr.trainable ? (E + kFreqCols - 1) / kFreqCols : 0;
                d_ans = d.off_ans; d_sse = d.P;
                d_w0 = d.off_w0; d_b0 = d.off_b0; d_w1 = d.off_w1; d_b1 = d.off_b1;
                w = w + d.off_ans;
                if (bid > nb_w + nb_x) return;
            }
        }
        partial = member_ptr(partial, wsb); grad_x = member_ptr(grad_x, wsb); pred = member_ptr(pred, wsb);
        gmap = member_ptr(gmap, wsb);
        fp.rec = member_ptr(fp.rec, wsb); fp.srec = member_ptr(fp.srec, wsb); fp.gmap = member_ptr(fp.gmap, wsb);
        w = member_ptr(w, pb);
        adam.p = member_ptr(adam.p, pb); adam.m = member_ptr(adam.m, pb); adam.v = member_ptr(adam.v, pb);
        y = member_ptr(y, m * ms.rows * (long)sizeof(double));
        grad = member_ptr(grad, m * ms.grad * (long)sizeof(double));
        // (enc stays as given -- its segments are indexed at run time, a modified copy would live in private memory: the
        // frequency blocks move their input pointer themselves, and nothing here reads the encoding weights)
    }
    __shared__ double acc[kRedThreads];
    __shared__ double acc2[kRedThreads];
    __shared__ int dp_failed;
    double *dp_loc = nullptr, *dp_xch = nullptr;
    long* dp_idx = nullptr;
    int* dp_count = nullptr;
    if constexpr (DP) {
        __shared__ double loc[kDpBlockValues], xch[kDpBlockValues * QHEA_DP_MAX_RANKS];
        __shared__ long idx[kDpBlockValues];
        __shared__ int count;
        dp_loc = loc; dp_xch = xch; dp_idx = idx; dp_count = &count;
    }
    const DpX* dp = DP ? &dpx : nullptr;
    QHEA_STAMP(0);
#ifdef QHEA_REDUCE_STAMPS
    const unsigned long long st0 = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (FUSE) if (bid < nb_w) {           // (block-uniform)
        __shared__ GateZ fgz[kFuseMaxLd][QHEA_MAX_QUBITS];     // the decompositions of the block's nbk x ld <= 2 sub-layers
        __shared__ double accbig[2 * kRedThreads];
        const double pn = reduce_xyz_block(bid, n, blk, kw, nwaves, partial, w, grad + gm.off_ans, accbig, acc, hdr->status != 0,
                                           gmap, &adam, gm.off_ans, fp.nbk * fp.ld * kw, dp, &dp_failed, dp_loc, dp_xch);
        QHEA_STAMP(3);
        // The next step's records.  Sincos and decomposition per gate in the lanes that have just updated its angles (wave 0:
        // lane 3q + k of sub-layer column group sl owns angle k of gate q), with no barrier: the lane of an angle takes the
        // (cos, sin) of its half angle, the gate's k = 0 lane gathers the other two by wave shuffles and decomposes the gate --
        // the functions and operands of prep_layer_body, so the records are bitwise those of prep_zyz_kernel.  Then one
        // barrier, and the record groups multiply phasors.
        const int tid = (int)threadIdx.x, lk = __builtin_ctz(kw), s0 = bid * fp.nbk * fp.ld, per = 1 + fp.ld;
        const int sl = tid >> lk, r = tid & (kw - 1), q = r / 3, k3 = r - 3 * q;
        const bool tri = tid < fp.nbk * fp.ld * kw && r < 3 * n && s0 + sl < blk;     // (reduce_xyz_block's `tri` lanes)
        double sn = 0.0, cn = 1.0;
        if (tri) fast_sincos(0.5 * pn, &sn, &cn);
        QHEA_STAMP(5);
        const double2 hb = make_double2(__shfl_down(cn, 1), __shfl_down(sn, 1));
        const double2 hc = make_double2(__shfl_down(cn, 2), __shfl_down(sn, 2));
        if (tri && k3 == 0) {
            const GateZ gz = gate_zyz(make_double2(cn, sn), hb, hc);
            fgz[sl][q] = gz;
            const int cq = sl >= fp.ld ? 1 : 0, g = sl - cq * fp.ld;      // sub-layer g of the block's circuit block cq
            const LayerInfo before = g == 0 ? LayerInfo{0, 0, n} : LayerInfo{1, s0 + sl - 1, 0};
            gate_zyz_stores(gz, before, n, (bid * fp.nbk + cq) * per + 1 + g, s0 + sl, q, fp.rec, fp.srec, fp.gmap);
        }
        QHEA_STAMP(6);
        __syncthreads();
        QHEA_STAMP(4);
        const int grp = tid >> 6, j = tid & 63;
        // record groups of 64 threads: for each of the reduce block's nbk circuit blocks, its ld sub-layers' records and the
        // FOLLOWING chunk's record (whose diagonal takes this block's last sub-layer through the ring)
        const bool act = grp < fp.nbk * per;
        const int cq = grp >= per ? 1 : 0;                 // (grp / per for the active groups: nbk <= 2)
        const int cb = bid * fp.nbk + cq, g = grp - cq * per;
        const int l = act ? (g < fp.ld ? cb * per + 1 + g : (cb + 1) * per) : 0;
        // (block-unrolled shapes, zyz_fast_ld: layer cb * per is circuit block cb's full RX chunk, the ld layers after it its
        // sub-layers cb * ld ..; record L, after the last sub-layer, has no layer of its own)
        const LayerInfo none{2, 0, 0}, chunk{0, 0, n};
        const LayerInfo cur = !act ? chunk : g < fp.ld ? LayerInfo{1, cb * fp.ld + g, 0} : (l < fp.L ? chunk : none);
        const LayerInfo prev = !act ? none : g == 0 ? chunk : LayerInfo{1, cb * fp.ld + g - 1, 0};
        const int zi = act ? cq * fp.ld + g : 0;           // (the group's sub-layers' gates: zc = this record's, zp = the one before)
        prep_layer_records(cur, prev, n, l, act ? j : 64, fgz[cur.kind == 1 ? zi : 0], fgz[prev.kind == 1 ? zi - 1 : 0],
                           fp.rec, fp.srec);
#ifdef QHEA_REDUCE_STAMPS
        if (threadIdx.x == 0 && bid == 30) {
            const unsigned long long e = __builtin_amdgcn_s_memtime();
            const unsigned long long* t = qhea_stamps;
            printf("reduce block 30: prologue %llu, first slice %llu | loads+slice sums %llu | tree %llu | finish+adam (thread 0) %llu | sincos %llu | decomposition %llu | barrier %llu | phasors+stores %llu | total %llu clk\n",
                   t[7] - t[0], t[8] - t[7], t[1] - t[0], t[2] - t[1], t[3] - t[2], t[5] - t[3], t[6] - t[5], t[4] - t[6], e - t[4], e - t[0]);
        }
#endif
        return;
    }
    // hand-off overrun in the circuit kernel: NaN out, no parameter update.  The word is only USED at the end of each
    // branch: nothing that is loaded before the sums depends on it, so its round trip overlaps theirs.
    const unsigned status = hdr->status;
    const double kNaN = std::numeric_limits<double>::quiet_NaN();
    if (bid < nb_w) {
        reduce_xyz_block(bid, n, blk, kw, nwaves, partial, w, grad + g_ans(), acc, acc2, status != 0, gmap, &adam, g_ans(),
                         0, dp, &dp_failed, dp_loc, dp_xch);
    } else if (bid < nb_w + nb_x) {
        const int j = threadIdx.x % kFreqCols, slice = threadIdx.x / kFreqCols;
        const int e = (bid - nb_w) * kFreqCols + j;
        double s0 = 0.0, s1 = 0.0;
        int si = 0, ee = e;
        if (e < E) {
            si = e < nc0() ? 0 : 1;
            if (si) ee = e - nc0();
        }
        // The segment's GradMap entries and input, chosen by a select between both segments' values: indexed by the run-time si
        // they were loads from the kernel arguments' memory -- a dependent round trip before the first load of the sums (the
        // input), and one after them before each store (the GradMap entries, read where they were used).
        long ow, ob;
        if constexpr (DEPTH) { ow = si ? d_w1 : d_w0; ob = si ? d_b1 : d_b0; }
        else { ow = si ? gm.off_w[1] : gm.off_w[0]; ob = si ? gm.off_b[1] : gm.off_b[0]; }
        auto g_w = [ow]() -> long { return ow; };
        auto g_b = [ob]() -> long { return ob; };
        const bool mine = slice == 0 && e < E && g_w() >= 0;
        // the lane that updates column e's bias and weight loads their Adam state now: it travels with the sums, not after them
        double pb = 0.0, mb = 0.0, vb = 0.0, pw = 0.0, mw = 0.0, vw = 0.0;
        if (mine && adam.p) {
            pb = adam.p[g_b() + ee]; mb = adam.m[g_b() + ee]; vb = adam.v[g_b() + ee];
            pw = adam.p[g_w() + ee]; mw = adam.m[g_w() + ee]; vw = adam.v[g_w() + ee];
        }
        if (e < E) {
            const int width = si ? enc.seg[1].width : enc.seg[0].width;
            const double* __restrict__ in = (si ? enc.seg[1].in : enc.seg[0].in) + mem * ms.rows * width + ee % width;
            const double* __restrict__ gx = grad_x + e;
            long b = slice;
            for (; b + 15L * kFreqSlices < B; b += 16L * kFreqSlices) {    // 32 loads in flight per thread: B = 1024 in ONE round trip
                double g[16], v[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    g[i] = gx[(b + (long)i * kFreqSlices) * E];
                    v[i] = in[(b + (long)i * kFreqSlices) * width];
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) { s0 += g[i]; s1 += g[i] * v[i]; }
            }
            for (; b + 7L * kFreqSlices < B; b += 8L * kFreqSlices) {      // 16 loads in flight per thread
                double g[8], v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    g[i] = gx[(b + (long)i * kFreqSlices) * E];
                    v[i] = in[(b + (long)i * kFreqSlices) * width];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) { s0 += g[i]; s1 += g[i] * v[i]; }
            }
            for (; b < B; b += kFreqSlices) {
                const double g = gx[b * E];
                s0 += g;
                s1 += g * in[b * width];
            }
        }
#ifdef QHEA_REDUCE_STAMPS
        const unsigned long long f_loads = __builtin_amdgcn_s_memtime();
#endif
        acc[slice * kFreqCols + j] = s0; acc2[slice * kFreqCols + j] = s1;
        __syncthreads();
        // slices combined in two fixed-order stages (kFreqStage interleaved groups, then those), as reduce_xyz_block does;
        // both stages run in wave 0 (slices < kFreqStage are its lanes), so the second takes the first's sums by wave shuffles
        static_assert(kFreqStage * kFreqCols == 64, "the frequency blocks' first-stage sums are wave 0's lanes");
        double u0 = 0.0, u1 = 0.0;
        if (slice < kFreqStage) {       // (unrolled: the LDS reads issued together, the additions in the loop's order)
            double a0[kFreqSlices / kFreqStage], a1[kFreqSlices / kFreqStage];
#pragma unroll
            for (int m = 0; m < kFreqSlices / kFreqStage; ++m) {
                a0[m] = acc[(slice + m * kFreqStage) * kFreqCols + j]; a1[m] = acc2[(slice + m * kFreqStage) * kFreqCols + j];
            }
#pragma unroll
            for (int m = 0; m < kFreqSlices / kFreqStage; ++m) { u0 += a0[m]; u1 += a1[m]; }
        }
        double t0 = 0.0, t1 = 0.0;
        bool skip = status != 0;
#pragma unroll
        for (int i = 0; i < kFreqStage; ++i) {          // (every lane shuffles; the `mine` lanes' sums are the ones used)
            const double x0 = __shfl(u0, i * kFreqCols + j), x1 = __shfl(u1, i * kFreqCols + j);
            t0 += x0; t1 += x1;
        }
        if (mine && skip) t0 = t1 = kNaN;
        if constexpr (DP) {
            // the block's exchanged values, compacted: (bias, weight) gradient of every column of a trainable segment (the
            // `mine` threads are lanes 0 .. kFreqCols-1 of wave 0)
            const unsigned long long bal = __ballot(mine);
            const int pos = __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull));
            if (threadIdx.x == 0) { dp_failed = 0; *dp_count = 2 * __popcll(bal); }
            if (mine) {
                dp_loc[2 * pos] = t0; dp_loc[2 * pos + 1] = t1;
                dp_idx[2 * pos] = g_b() + ee; dp_idx[2 * pos + 1] = g_w() + ee;
            }
            __syncthreads();
            const bool ok = dpx_exchange_block(dpx, *dp_count, dp_loc, [dp_idx](int i) { return dp_idx[i]; }, dp_xch, &dp_failed);
            if (mine) {
                t0 = ok ? dpx_sum(dpx, dp_xch, 2 * pos) : kNaN;
                t1 = ok ? dpx_sum(dpx, dp_xch, 2 * pos + 1) : kNaN;
                skip = !(t0 == t0 && t1 == t1);
            }
        }
        if (mine) {
            store_through(&grad[g_b() + ee], t0);
            store_through(&grad[g_w() + ee], t1);
            if (adam.p && !skip) {
                adam_update_pre(adam, g_b() + ee, t0, pb, mb, vb);
                adam_update_pre(adam, g_w() + ee, t1, pw, mw, vw);
            }
        }
#ifdef QHEA_REDUCE_STAMPS
        if (threadIdx.x == 0 && bid == nb_w)
            printf("reduce freq block: loads+sums %llu | stages+adam %llu | total %llu clk\n", f_loads - st0,
                   __builtin_amdgcn_s_memtime() - f_loads, __builtin_amdgcn_s_memtime() - st0);
#endif
    } else {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        double pb = 0.0, mb = 0.0, vb = 0.0;           // the bias's Adam state, loaded with the sums (frequency blocks: the same)
        if (threadIdx.x == 0 && gm.off_bias >= 0 && adam.p) { pb = adam.p[gm.off_bias]; mb = adam.m[gm.off_bias]; vb = adam.v[gm.off_bias]; }
        for (long b = threadIdx.x; b < B; b += kRedThreads) {
            const double r = pred[b] - y[b];
            s0 += r * r; s1 += r; s2 += y[b] * y[b];
        }
        __shared__ double red3[kRedThreads];
        acc[threadIdx.x] = s0; acc2[threadIdx.x] = s1; red3[threadIdx.x] = s2;
        __syncthreads();
        for (int stride = kRedThreads / 2; stride > 0; stride >>= 1) {
            if ((int)threadIdx.x < stride) {
                acc[threadIdx.x] += acc[threadIdx.x + stride];
                acc2[threadIdx.x] += acc2[threadIdx.x + stride];
                red3[threadIdx.x] += red3[threadIdx.x + stride];
            }
            __syncthreads();
        }
        const bool poisoned = status != 0;
        double sse = poisoned ? kNaN : acc[0], sy2 = red3[0], gbias = poisoned ? kNaN : 2.0 * inv_bt * acc2[0];
        bool skip = poisoned;
        if constexpr (DP) {
            if (threadIdx.x == 0) {
                dp_failed = 0;
                dp_loc[0] = sse; dp_idx[0] = g_sse();
                dp_loc[1] = sy2; dp_idx[1] = g_sse() + 1;
                if (gm.off_bias >= 0) { dp_loc[2] = gbias; dp_idx[2] = gm.off_bias; }
                *dp_count = gm.off_bias >= 0 ? 3 : 2;
            }
            __syncthreads();
            const bool ok = dpx_exchange_block(dpx, *dp_count, dp_loc, [dp_idx](int i) { return dp_idx[i]; }, dp_xch, &dp_failed);
            if (threadIdx.x == 0) {
                sse = ok ? dpx_sum(dpx, dp_xch, 0) : kNaN;
                sy2 = ok ? dpx_sum(dpx, dp_xch, 1) : kNaN;
                if (gm.off_bias >= 0) gbias = ok ? dpx_sum(dpx, dp_xch, 2) : kNaN;
                skip = !(gbias == gbias) || !ok;
            }
        }
        if (threadIdx.x == 0) {
            store_through(&grad[g_sse()], sse);
            store_through(&grad[g_sse() + 1], sy2);
            if (gm.off_bias >= 0) {
                store_through(&grad[gm.off_bias], gbias);
                if (adam.p && !skip) adam_update_pre(adam, gm.off_bias, gbias, pb, mb, vb);
            }
        }
#ifdef QHEA_REDUCE_STAMPS
        if (threadIdx.x == 0) printf("reduce tail block: %llu clk\n", __builtin_amdgcn_s_memtime() - st0);
#endif
    }
}

// Depth sweeps: prep_model_kernel for member blockIdx.y, whose shape (depth_map) comes from its MemberRec -- gate table of its
// blk sub-layers from its angles, (cos, sin) of its E encoding columns with its frequency layers or its fixed scale.  params:
// member 0's row (rows ms.params doubles apart), gates / cs: member 0's slice, enc: segment inputs and widths only.  The grid
// is sized for the largest member; threads beyond the member's entries write nothing.
__global__ void prep_model_depth_kernel(int n, DepthRed dr, const double* __restrict__ params, double4* __restrict__ gates,
                                        long B, EncDesc enc, double2* __restrict__ cs, WorkspaceHeader* hdr, const char* mrec,
                                        MemberStride ms) {
    const long m = blockIdx.y, wsb = m * ms.ws;
    const ConstMemberRec mr = (ConstMemberRec)member_ptr(reinterpret_cast<const MemberRec*>(mrec), wsb);
    const DepthMap d = depth_map(n, dr.quanonet != 0, dr.trainable != 0, mr->depth[0], mr->depth[1], dr.ld0, dr.ld1);
    const double* __restrict__ p = params + m * ms.params;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid == 0 && m == 0) header_init(hdr);
    const long ng = (long)(d.blk + 2) * n;
    if (tid < ng) {
        prep_gate_entry(n, d.blk, p + d.off_ans, member_ptr(gates, wsb), tid);
    } else if (tid - ng < B * d.E) {
        const long t = tid - ng;
        const long b = t / d.E;
        int e = (int)(t % d.E);
        const int si = e < d.nc0 ? 0 : 1;
        if (si) e -= d.nc0;
        const EncSeg& sg = enc.seg[si];
        const double v = sg.in[(b + m * ms.rows) * sg.width + e % sg.width];
        const double x = dr.trainable ? v * p[(si ? d.off_w1 : d.off_w0) + e] + p[(si ? d.off_b1 : d.off_b0) + e] : v * mr->scale;
        double sn, cn;
        fast_sincos(0.5 * x, &sn, &cn);
        member_ptr(cs, wsb)[t] = make_double2(cn, sn);
    }
}

// Qubit sweeps: prep_model_depth_kernel for members of different n -- member blockIdx.y's n is its MemberRec::nq.  The grid is
// sized for the largest member.  The workgroup-resident kernels (n >= 10) read the same tables as the wave-resident ones.
__global__ void prep_model_qubit_kernel(DepthRed dr, const double* __restrict__ params, double4* __restrict__ gates,
                                        long B, EncDesc enc, double2* __restrict__ cs, WorkspaceHeader* hdr, const char* mrec,
                                        MemberStride ms) {
    const long m = blockIdx.y, wsb = m * ms.ws;
    const ConstMemberRec mr = (ConstMemberRec)member_ptr(reinterpret_cast<const MemberRec*>(mrec), wsb);
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid == 0 && m == 0) header_init(hdr);
    const int n = mr->nq;
    const DepthMap d = depth_map(n, dr.quanonet != 0, dr.trainable != 0, mr->depth[0], mr->depth[1], dr.ld0, dr.ld1);
    const double* __restrict__ p = params + m * ms.params;
    const long ng = (long)(d.blk + 2) * n;
    if (tid < ng) {
        prep_gate_entry(n, d.blk, p + d.off_ans, member_ptr(gates, wsb), tid);
    } else if (tid - ng < B * d.E) {
        const long t = tid - ng;
        const long b = t / d.E;
        int e = (int)(t % d.E);
        const int si = e < d.nc0 ? 0 : 1;
        if (si) e -= d.nc0;
        const EncSeg& sg = enc.seg[si];
        const double v = sg.in[(b + m * ms.rows) * sg.width + e % sg.width];
        const double x = dr.trainable ? v * p[(si ? d.off_w1 : d.off_w0) + e] + p[(si ? d.off_b1 : d.off_b0) + e] : v * mr->scale;
        double sn, cn;
        fast_sincos(0.5 * x, &sn, &cn);
        member_ptr(cs, wsb)[t] = make_double2(cn, sn);
    }
}

// Diagnostic: the clock the shader engines actually run at, measured inside a kernel.  Every workgroup times a dependent fp64
// FMA chain with s_memtime (shader-clock ticks) against s_memrealtime (the constant 100 MHz counter); the ratio x 100 MHz is
// its in-kernel clock (MI355X_MICROARCH.md, clocks section: devices of one model differ by up to ~12 % there, which is the
// box-to-box spread of the latency-bound kernels here).  bench.py reports the median over the workgroups.
__global__ __launch_bounds__(64) void clock_probe_kernel(long iters, unsigned long long* out) {
    double x = 1.0 + 1e-9 * threadIdx.x, y = 1.0 - 1e-12;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (long i = 0; i < iters; ++i) x = fma(x, y, 1e-13);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = t1 - t0; out[2 * blockIdx.x + 1] = r1 - r0; }
    if (x == 123.456) out[0] = 0;                        // keep the chain
}

int model_info(const qhea_model_desc* d, ModelInfo& mi) {
    if (!d) return QHEA_EINVAL;
    if (d->ham_pauli < QHEA_PAULI_Z || d->ham_pauli > QHEA_PAULI_Y) return QHEA_EINVAL;
    const int n = d->n_qubits;
    if (n < QHEA_MIN_QUBITS || n > QHEA_MAX_QUBITS) return QHEA_EINVAL;
    for (int i = 0; i < 4; ++i) if (d->net[i] < 0) return QHEA_EINVAL;
    mi.n = n;
    mi.trainable = d->trainable_freq != 0;
    // block list: QuanONet = td x (n, tl) then bd x (n, bl) (core/quantum_circuits_tq.py:130-138); HEAQNN = depth x (n, ld)
    if (d->model == QHEA_MODEL_QUANONET) {
        if (d->branch_in <= 0 || d->trunk_in <= 0) return QHEA_EINVAL;
        mi.nb[0] = d->net[2]; mi.ld[0] = d->net[3]; mi.nb[1] = d->net[0]; mi.ld[1] = d->net[1];
        mi.width[0] = d->trunk_in; mi.width[1] = d->branch_in;   // x columns: trunk first (core/models_pt.py:164)
        mi.has_bias = true;
    } else if (d->model == QHEA_MODEL_HEAQNN) {
        if (d->branch_in <= 0) return QHEA_EINVAL;
        mi.nb[0] = d->net[0]; mi.ld[0] = d->net[1]; mi.nb[1] = 0; mi.ld[1] = 0;
        mi.width[0] = d->branch_in; mi.width[1] = 1;
        mi.has_bias = false;
    } else {
        return QHEA_EINVAL;
    }
    for (int g = 0; g < 2; ++g) {
        mi.enc_cols[g] = (long)mi.nb[g] * n;
        append_blocks(mi.sh, mi.nb[g], n, mi.ld[g]);             // (two runs at the most: never refused)
    }
    const int rc = finish_shape(n, (long)mi.nb[0] + mi.nb[1], mi.sh);
    if (rc != QHEA_OK) return rc;
    long p = 0;
    if (mi.has_bias) { mi.off_bias = p; p += 1; }             // nn.Module order: own parameter `bias` first
    if (mi.trainable) {                                        // then branch_freq, trunk_freq (QuanONet), quantum_layer
        for (int g = d->model == QHEA_MODEL_QUANONET ? 1 : 0; g >= 0; --g) {
            mi.off_w[g] = p; p += mi.enc_cols[g]; mi.off_b[g] = p; p += mi.enc_cols[g];
        }
    }
    mi.off_ans = p; p += mi.sh.blk * 3 * n;
    mi.P = p;
    return QHEA_OK;
}

GradMap grad_map(const ModelInfo& mi) {
    GradMap gm{};
    gm.off_ans = mi.off_ans; gm.off_bias = mi.off_bias; gm.off_sse = mi.P;
    for (int s = 0; s < 2; ++s) { gm.off_w[s] = mi.off_w[s]; gm.off_b[s] = mi.off_b[s]; }
    return gm;
}

// the run table of the depth and qubit sweeps: two runs of fixed (enc = n, ld); the counts are the members'
Runs two_runs(int n, int ld0, int ld1) {
    Runs r{};
    r.nruns = 2;
    r.enc[0] = r.enc[1] = n;
    r.ld[0] = ld0; r.ld[1] = ld1;
    return r;
}

// reduce blocks of a model of blk sub-layers and E encoding columns by role (reduce_model_kernel): ansatz blocks, frequency
// blocks, and the sse / bias block
struct RedBlocks {
    int nb_w, nb_x;
    int total() const { return nb_w + nb_x + 1; }
};
RedBlocks red_blocks(int n, long blk, long E, bool trainable) {
    const int kw = padded_3n(n);
    return RedBlocks{(int)((blk * kw + red_cols(kw) - 1) / red_cols(kw)), trainable ? (int)((E + kFreqCols - 1) / kFreqCols) : 0};
}

struct ModelLayout { Layout L; size_t off_gx, off_pred, total; };

ModelLayout make_model_layout(const ModelInfo& mi, int64_t B, int64_t Bd /* rows of the launch: R x B for an ensemble */) {
    ModelLayout M{};
    M.L = make_layout(mi.n, mi.sh, B, Bd);
    size_t p = M.L.total;
    M.off_gx = p;   p = align256(p + (size_t)B * mi.sh.E * sizeof(double));
    M.off_pred = p; p = align256(p + (size_t)B * sizeof(double));
    M.total = p;
    return M;
}
ModelLayout make_model_layout(const ModelInfo& mi, int64_t B) { return make_model_layout(mi, B, B); }

EncDesc make_enc(const qhea_model_desc* d, const ModelInfo& mi, const double* branch, const double* trunk,
                 const double* params) {
    EncDesc enc{};
    const double* in[2] = {d->model == QHEA_MODEL_QUANONET ? trunk : branch, branch};
    for (int s = 0; s < 2; ++s) {
        enc.seg[s].in = in[s];
        enc.seg[s].width = mi.width[s];
        enc.seg[s].ncols = (int)mi.enc_cols[s];
        enc.seg[s].scale = d->scale_coeff;
        enc.seg[s].w = (mi.trainable && mi.off_w[s] >= 0) ? params + mi.off_w[s] : nullptr;
        enc.seg[s].b = (mi.trainable && mi.off_b[s] >= 0) ? params + mi.off_b[s] : nullptr;
    }
    return enc;
}

int launch_prep_model(const qhea_model_desc* d, const ModelInfo& mi, int64_t B, const double* branch, const double* trunk,
                      const double* params, double4* gates, double2* cs, void* hdr, hipStream_t st) {
    const long total = (mi.sh.blk + 2) * mi.n + B * mi.sh.E;
    const int threads = 256;
    hipLaunchKernelGGL(prep_model_kernel, dim3((unsigned)((total + threads - 1) / threads)), dim3(threads), 0, st,
                       mi.n, (int)mi.sh.blk, params + mi.off_ans, gates, (long)B, (int)mi.sh.E,
                       make_enc(d, mi, branch, trunk, params), cs, static_cast<WorkspaceHeader*>(hdr));
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

// R-sequential ensemble fallback (qhea_model_ensemble_train_steps): member m > 0 ran on its own workspace slice, whose header
// took its status; the overrun is moved into slice 0's header, the one qhea_check_status reads
__global__ void status_fold_kernel(WorkspaceHeader* dst, WorkspaceHeader* src) {
    if (threadIdx.x == 0 && src->magic == kWsMagic && src->status != 0) {
        header_init(dst);
        dst->status |= src->status;
        src->status = 0;
    }
}

// bytes of one member's workspace slice for a step of `batch` rows in an R-member ensemble: enough for the one-launch path
// (kernels chosen for R x batch rows) and for the R-sequential one (chosen for batch rows)
size_t ensemble_slice_bytes(const ModelInfo& mi, int64_t R, int64_t batch) {
    const size_t a = make_model_layout(mi, batch, R * batch).total, b = make_model_layout(mi, batch).total;
    return a > b ? a : b;
}
// whether a step of `batch` rows of an R-member ensemble runs as one launch per kernel (member = blockIdx.y): the ZYZ kernels
bool ensemble_grid(const ModelInfo& mi, int64_t R, int64_t batch) { return make_model_layout(mi, batch, R * batch).L.zyz_bwd; }

// The members' hyper-parameters reach the device as kernel arguments: one launch per kMemberFill members and host call writes
// each member's MemberRec (hea_zyz.hpp) into its workspace slice -- no pageable copy, nothing retained, capturable.
constexpr int kMemberFill = 64;                 // 64 x 40 (depth sweeps: 48, qubit sweeps: 52) bytes of kernel arguments
struct MemberFill { qhea_member_hparams h[kMemberFill]; };
struct MemberFillDepth : MemberFill {           // depth sweeps: + the members' block counts (MemberRec::depth)
    int32_t depth[kMemberFill][2];
};
struct MemberFillQubit : MemberFillDepth {      // qubit sweeps: + the members' qubit counts (MemberRec::nq)
    int32_t nq[kMemberFill];
};
template <class F>
__global__ __launch_bounds__(kMemberFill) void member_fill_kernel(F f, int count, char* slice0, long slice_bytes,
                                                                  const double* diag0, long diag_stride) {
    const int i = threadIdx.x;
    if (i >= count) return;
    const qhea_member_hparams& h = f.h[i];
    MemberRec r;
    r.scale = h.scale_coeff; r.off = h.ham_offset; r.co = h.ham_coeff; r.lr = h.lr;
    r.diag = diag0 ? diag0 + (long)i * diag_stride : nullptr;
    r.pauli = h.ham_pauli; r.nq = 0;
    r.depth[0] = r.depth[1] = 0;
    if constexpr (std::is_base_of<MemberFillDepth, F>::value) { r.depth[0] = f.depth[i][0]; r.depth[1] = f.depth[i][1]; }
    if constexpr (std::is_same<F, MemberFillQubit>::value) r.nq = f.nq[i];
    *reinterpret_cast<MemberRec*>(slice0 + (long)i * slice_bytes + kMemberRecOffset) = r;
}
// The fill launches of members 0 .. n_models - 1 (slices of `slice` bytes from ws on; member m's diagonal Hamiltonian is
// diag0 + m * diag_stride, diag0 == nullptr: none): fill(f, i, m) sets element i of a launch's F from member m
template <class F, class Fill>
int fill_member_recs(int64_t n_models, char* ws, size_t slice, const double* diag0, int64_t diag_stride, hipStream_t st,
                     Fill fill) {
    for (int64_t m0 = 0; m0 < n_models; m0 += kMemberFill) {
        const int cnt = (int)(n_models - m0 < kMemberFill ? n_models - m0 : kMemberFill);
        F f{};
        for (int i = 0; i < cnt; ++i) fill(f, i, m0 + i);
        hipLaunchKernelGGL(member_fill_kernel<F>, dim3(1), dim3(kMemberFill), 0, st, f, cnt, ws + m0 * slice, (long)slice,
                           diag0 ? diag0 + m0 * diag_stride : nullptr, (long)diag_stride);
        if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    }
    return QHEA_OK;
}
// Qubit sweeps: the work lists (hea_qsweep.hpp: QsWork) reach the slices' list regions the same way, kWorkFill entries per launch
constexpr int kWorkFill = 256;                  // 2 KB of kernel arguments
struct WorkFill { int2 e[kWorkFill]; };
__global__ __launch_bounds__(kWorkFill) void work_fill_kernel(WorkFill f, int count, int k0, char* list0, long slice_bytes, int per) {
    const int i = threadIdx.x;
    if (i >= count) return;
    const int k = k0 + i;
    *reinterpret_cast<int2*>(list0 + (long)(k / per) * slice_bytes + (long)(k % per) * (long)sizeof(int2)) = f.e[i];
}

// The descriptor member m trains as: the shape of `desc`, m's read-out and fixed scale
inline qhea_model_desc member_desc(const qhea_model_desc& d, const qhea_member_hparams& h) {
    qhea_model_desc m = d;
    m.scale_coeff = h.scale_coeff; m.ham_offset = h.ham_offset; m.ham_coeff = h.ham_coeff; m.ham_pauli = h.ham_pauli;
    return m;
}

}  // namespace qhea

using namespace qhea;

extern "C" {

int qhea_version(void) { return 670; }

const char* qhea_strerror(int code) {
    switch (code) {
        case QHEA_OK: return "ok";
        case QHEA_EINVAL: return "invalid argument";
        case QHEA_EUNSUPPORTED: return "unsupported circuit shape";
        case QHEA_EWORKSPACE: return "workspace missing or too small";
        case QHEA_ELAUNCH: return "HIP launch/runtime failure";
        case QHEA_ENODEVICE: return "no usable HIP device";
        case QHEA_EPIPELINE: return "a pipelined backward kernel overran a hand-off wait: results of that call are invalid";
        case QHEA_EEXCHANGE: return "a data-parallel exchange did not hear from every rank in time: that step's update was skipped";
        default: return "unknown error";
    }
}

int qhea_profile_next_circuit_kernel(void* start_event, void* stop_event) {
    g_ev_start = static_cast<hipEvent_t>(start_event);
    g_ev_stop = static_cast<hipEvent_t>(stop_event);
    return QHEA_OK;
}

int qhea_clock_probe(int n_workgroups, int64_t iters, unsigned long long* ticks /*DEVICE [2 * n_workgroups]*/, void* stream) {
    if (n_workgroups < 1 || iters < 1 || !ticks) return QHEA_EINVAL;
    hipLaunchKernelGGL(clock_probe_kernel, dim3((unsigned)n_workgroups), dim3(64), 0, static_cast<hipStream_t>(stream), (long)iters, ticks);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

int qhea_set_backward_variant(int variant) {
    if (variant < QHEA_BWD_AUTO || variant > QHEA_BWD_ZSNAP) return QHEA_EINVAL;
    g_bwd_variant.store(variant, std::memory_order_relaxed);
    return QHEA_OK;
}

int qhea_check_status(void* workspace, size_t workspace_bytes, void* stream) {
    if (!workspace || workspace_bytes < kHeaderBytes) return QHEA_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    WorkspaceHeader h{};
    if (hipMemcpyAsync(&h, workspace, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess) return QHEA_ELAUNCH;
    if (hipStreamSynchronize(st) != hipSuccess) return QHEA_ELAUNCH;
    if (h.magic != kWsMagic || h.status == 0) return QHEA_OK;         // never used, or clean
    if (hipMemsetAsync(&static_cast<WorkspaceHeader*>(workspace)->status, 0, sizeof(int), st) != hipSuccess)
        return QHEA_ELAUNCH;
    return QHEA_EPIPELINE;
}

int qhea_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

size_t qhea_workspace_bytes(int n_qubits, int n_blocks, const int32_t* enc_per_block,
                            const int32_t* ld_per_block, int64_t batch) {
    Shape sh;
    if (make_shape(n_qubits, n_blocks, enc_per_block, ld_per_block, sh) != QHEA_OK || batch < 0) return 0;
    return make_layout(n_qubits, sh, batch).total;
}

int qhea_forward(int n_qubits, int n_blocks, const int32_t* enc_per_block, const int32_t* ld_per_block,
                 int64_t batch, const double* x, const double* w, double ham_offset, double ham_coeff,
                 const double* ham_diag, int ham_pauli, double* out, double* state_out, void* workspace,
                 size_t workspace_bytes, void* stream) {
    Shape sh;
    int rc = make_shape(n_qubits, n_blocks, enc_per_block, ld_per_block, sh);
    if (rc != QHEA_OK) return rc;
    if (batch < 0 || !pauli_ok(ham_pauli, ham_diag)) return QHEA_EINVAL;
    if (batch == 0) return QHEA_OK;
    if (!out || (sh.E > 0 && !x) || (sh.blk > 0 && !w)) return QHEA_EINVAL;
    const Layout L = make_layout(n_qubits, sh, batch);
    if (!workspace || workspace_bytes < L.total) return QHEA_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const FwdKernel k = fwd_kernel_for(L.in, CallTraits{ham_pauli});
    if (zyz_family(k)) {
        rc = launch_prep_zyz(n_qubits, sh, w, ws, L, st);
        if (rc != QHEA_OK) return rc;
        return launch_zyz_forward(k, n_qubits, sh, batch, L, ws, AngleSrc{x, EncDesc{}}, ham_offset, ham_coeff, ham_diag, ham_pauli,
                                  out, state_out, nullptr, st);
    }
    rc = launch_prep(n_qubits, sh, batch, w, x, ws, L, st);
    if (rc != QHEA_OK) return rc;
    return launch_table_forward(k, n_qubits, sh, batch, L, ws, ham_offset, ham_coeff, ham_diag, ham_pauli, out, state_out, nullptr, st);
}

int qhea_backward(int n_qubits, int n_blocks, const int32_t* enc_per_block, const int32_t* ld_per_block,
                  int64_t batch, const double* x, const double* w, double ham_offset, double ham_coeff,
                  const double* ham_diag, int ham_pauli, const double* g, const double* state_in, double* out,
                  double* grad_x, double* grad_w, void* workspace, size_t workspace_bytes, void* stream) {
    Shape sh;
    int rc = make_shape(n_qubits, n_blocks, enc_per_block, ld_per_block, sh);
    if (rc != QHEA_OK) return rc;
    if (batch < 0 || !pauli_ok(ham_pauli, ham_diag)) return QHEA_EINVAL;
    if ((sh.blk > 0 && (!w || !grad_w))) return QHEA_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (batch == 0) {
        if (sh.blk > 0 && hipMemsetAsync(grad_w, 0, sizeof(double) * sh.blk * 3 * n_qubits, st) != hipSuccess)
            return QHEA_ELAUNCH;
        return QHEA_OK;
    }
    if (!g || (sh.E > 0 && (!x || !grad_x))) return QHEA_EINVAL;
    const Layout L = make_layout(n_qubits, sh, batch);
    if (!workspace || workspace_bytes < L.total) return QHEA_EWORKSPACE;
    char* ws = static_cast<char*>(workspace);
    double* partial = reinterpret_cast<double*>(ws + L.off_part);
    const BwdKernel k = bwd_kernel_for(L.in, n_qubits, CallTraits{ham_pauli, state_in != nullptr});
    if (L.zyz_bwd) {
        rc = launch_prep_zyz(n_qubits, sh, w, ws, L, st);
        if (rc == QHEA_OK)
            rc = launch_zyz_backward(k, n_qubits, sh, batch, L, ws, AngleSrc{x, EncDesc{}}, ham_offset, ham_coeff, ham_diag,
                                     ham_pauli, g, state_in, nullptr, nullptr, 0.0, out, grad_x, partial, st);
    } else {
        rc = launch_prep(n_qubits, sh, batch, w, x, ws, L, st);
        if (rc == QHEA_OK)
            rc = launch_table_backward(k, n_qubits, sh, batch, L, ws, ham_offset, ham_coeff, ham_diag, ham_pauli, g, state_in,
                                       nullptr, nullptr, 0.0, out, grad_x, partial, st);
    }
    if (rc != QHEA_OK) return rc;
    if (sh.blk > 0) {       // (the ZYZ kernels' sums are taken before the gate's last RZ: through gmap)
        const int kw = padded_3n(n_qubits);
        const long ncols = sh.blk * kw;
        hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((ncols + red_cols(kw) - 1) / red_cols(kw))), dim3(kRedThreads), 0, st,
                           n_qubits, (int)sh.blk, kw, L.nwaves, partial, w, grad_w, reinterpret_cast<const WorkspaceHeader*>(ws),
                           L.zyz_bwd ? reinterpret_cast<const double*>(ws + L.off_gmap) : nullptr);
    }
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

int64_t qhea_model_param_count(const qhea_model_desc* desc) {
    ModelInfo mi;
    const int rc = model_info(desc, mi);
    return rc == QHEA_OK ? (int64_t)mi.P : (int64_t)rc;
}

size_t qhea_model_workspace_bytes(const qhea_model_desc* desc, int64_t batch) {
    ModelInfo mi;
    if (model_info(desc, mi) != QHEA_OK || batch < 0) return 0;
    return make_model_layout(mi, batch).total;
}

// records_ready (qhea_model_forward_chunks only): an earlier chunk of the same call has left this layout's layer records
static int model_forward_impl(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                              const double* params, const double* ham_diag, double* pred, void* workspace,
                              size_t workspace_bytes, void* stream, bool records_ready) {
    ModelInfo mi;
    int rc = model_info(desc, mi);
    if (rc != QHEA_OK) return rc;
    if (batch < 0 || !pauli_ok(desc->ham_pauli, ham_diag)) return QHEA_EINVAL;
    if (batch == 0) return QHEA_OK;
    if (!branch || !params || !pred || (desc->model == QHEA_MODEL_QUANONET && !trunk)) return QHEA_EINVAL;
    const ModelLayout M = make_model_layout(mi, batch);
    if (!workspace || workspace_bytes < M.total) return QHEA_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const EncDesc enc = make_enc(desc, mi, branch, trunk, params);
    const double* bias = mi.has_bias ? params + mi.off_bias : nullptr;
    const FwdKernel k = fwd_kernel_for(M.L.in, CallTraits{desc->ham_pauli});
    if (zyz_family(k)) {
        if (!records_ready) {
            rc = launch_prep_zyz(mi.n, mi.sh, params + mi.off_ans, ws, M.L, st);
            if (rc != QHEA_OK) return rc;
        }
        return launch_zyz_forward(k, mi.n, mi.sh, batch, M.L, ws, AngleSrc{nullptr, enc}, desc->ham_offset, desc->ham_coeff, ham_diag,
                                  desc->ham_pauli, pred, nullptr, bias, st);
    }
    rc = launch_prep_model(desc, mi, batch, branch, trunk, params, reinterpret_cast<double4*>(ws + M.L.off_U),
                           reinterpret_cast<double2*>(ws + M.L.off_cs), ws, st);
    if (rc != QHEA_OK) return rc;
    return launch_table_forward(k, mi.n, mi.sh, batch, M.L, ws, desc->ham_offset, desc->ham_coeff, ham_diag, desc->ham_pauli, pred,
                                nullptr, bias, st);
}

// the reduce kernel can write the next step's records: ZYZ kernels on a block-unrolled shape whose reduce block (ld x kw
// columns) divides the block size
// circuit blocks per reduce block of the fused path, 0 = the shape is not eligible.  A reduce block of 16 or 32 columns adds
// every column exactly as the plain 16-column blocks do; it must own whole circuit blocks: ld x kw = 16 or 32 columns is one
// block, 8 columns (n = 2 with one sub-layer per block: the shipped Antideriv Q2 Net5-1-5-1 model) are half a reduce block, so
// two consecutive circuit blocks share one (an even number of blocks is needed).
static int model_fuse_blocks(const ModelInfo& mi, const Layout& L) {
    const int ld = mi.sh.fast_ld, kw = padded_3n(mi.n);
    if (!L.zyz_bwd || ld < 1 || ld > kFuseMaxLd || mi.sh.blk % ld != 0) return 0;
    const int cols = ld * kw;
    if (cols == 16 || cols == 32) return 1;
    if (cols == 8 && (mi.sh.blk / ld) % 2 == 0) return 2;
    return 0;
}
static bool model_fuse_eligible(const ModelInfo& mi, const Layout& L) { return model_fuse_blocks(mi, L) != 0; }

// reduce launch of the model-level calls: FUSE = also writes the next step's records, dpx = exchanges with the peer ranks
static int launch_reduce_model(const RedBlocks& rb, hipStream_t st, const ModelInfo& mi, long nwaves, const double* partial,
                               const double* params, const StepView& v, const EncDesc& enc, const double* gx, const double* pr,
                               const AdamArgs& adam, const char* ws, const double* gmap, const FusePrep& fp, const DpX* dpx,
                               int R = 1, const MemberStride& ms = MemberStride{}, const MemberLr* mlr = nullptr) {
    const DpX none{};
    const DpX& dx = dpx ? *dpx : none;
    const dim3 g((unsigned)rb.total(), (unsigned)R), b(kRedThreads);
    const WorkspaceHeader* hdr = reinterpret_cast<const WorkspaceHeader*>(ws);
    const MemberLr ml = mlr ? *mlr : MemberLr{};
    const GradMap gm = grad_map(mi);
#define QHEA_LAUNCH_REDUCE(F, D, M)                                                                                       \
    hipLaunchKernelGGL((reduce_model_kernel<F, D, M>), g, b, 0, st, mi.n, (int)mi.sh.blk, padded_3n(mi.n), nwaves, partial, \
                       params + mi.off_ans, (long)v.nb, (int)mi.sh.E, enc, gx, pr, v.y, v.inv_bt, gm, rb.nb_w, rb.nb_x, v.grad, \
                       adam, hdr, gmap, fp, dx, ms, ml)
    if (mlr) { if (fp.ld != 0) QHEA_LAUNCH_REDUCE(true, false, true); else QHEA_LAUNCH_REDUCE(false, false, true); }
    else if (fp.ld != 0) { if (dpx) QHEA_LAUNCH_REDUCE(true, true, false); else QHEA_LAUNCH_REDUCE(true, false, false); }
    else                 { if (dpx) QHEA_LAUNCH_REDUCE(false, true, false); else QHEA_LAUNCH_REDUCE(false, false, false); }
#undef QHEA_LAUNCH_REDUCE
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

// a data-parallel reduce launch needs every block resident at once (its blocks wait for the peers' blocks) and a flag
// per block in the exchange buffers
// (a reduce block exchanges at most its column count of values -- 64 for n = 12 -- or 2 x kFreqCols, or 3)
static_assert(kDpBlockValues >= 64 && kDpBlockValues >= 2 * kFreqCols, "dpx_exchange_block's LDS arrays");
static bool dp_blocks_ok(int nblocks) { return nblocks <= kDpMaxBlocks && nblocks <= simd_count() / 4; }      // (all resident: blocks wait for their peers)

// One step (v: its rows, gradient row and residual weight) of the model-level calls.
static int model_loss_grad_impl(const qhea_model_desc* desc, const StepView& v, const double* params, const double* ham_diag,
                                double* pred, void* workspace, size_t workspace_bytes, void* stream,
                                const AdamArgs& adam, bool records_ready = false, bool records_for_next = false,
                                const DpX* dpx = nullptr, int R = 1, const MemberStride& ms = MemberStride{},
                                const MemberLr* mlr = nullptr) {
    // records_ready / records_for_next (qhea_model_train_steps only): the previous step's reduce kernel has written this
    // step's layer records / this step's reduce kernel writes the next step's (FusePrep).  dpx (qhea_model_dp_train_steps):
    // the reduce kernel's blocks exchange their gradients with the peer ranks before they update.  R, ms
    // (qhea_model_ensemble_train_steps only): R members in every launch, member 0's pointers given, workspace_bytes = one slice;
    // the kernels are chosen for R x batch rows.  mlr (R > 1): the members' MemberRecs (read-out, scale, lr) are in their slices.
    ModelInfo mi;
    int rc = model_info(desc, mi);
    if (rc != QHEA_OK) return rc;
    const int64_t batch = v.nb;
    if (batch < 0 || !v.grad || !pauli_ok(desc->ham_pauli, ham_diag)) return QHEA_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (batch == 0) {
        if (dpx) return QHEA_EUNSUPPORTED;                      // (an empty shard still owes the peers its zeros: caller's path)
        return hipMemsetAsync(v.grad, 0, sizeof(double) * (mi.P + 2), st) == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
    }
    if (!v.branch || !params || !v.y || (desc->model == QHEA_MODEL_QUANONET && !v.trunk)) return QHEA_EINVAL;
    if (R > 1 && !mlr) return QHEA_EINVAL;                      // (the member kernels read every member's MemberRec)
    const ModelLayout M = make_model_layout(mi, batch, R * batch);
    if (!workspace || workspace_bytes < M.total) return QHEA_EWORKSPACE;
    char* ws = static_cast<char*>(workspace);
    const EncDesc enc = make_enc(desc, mi, v.branch, v.trunk, params);
    double* gx = reinterpret_cast<double*>(ws + M.off_gx);
    double* pr = pred ? pred : reinterpret_cast<double*>(ws + M.off_pred);
    double* partial = reinterpret_cast<double*>(ws + M.L.off_part);
    RedBlocks rb = red_blocks(mi.n, mi.sh.blk, mi.sh.E, mi.trainable);
    FusePrep fp{};
    const double* bias = mi.has_bias ? params + mi.off_bias : nullptr;
    const BwdKernel k = bwd_kernel_for(M.L.in, mi.n, CallTraits{desc->ham_pauli, false, R});
    if (M.L.zyz_bwd) {
        if (records_for_next) {
            if (!model_fuse_eligible(mi, M.L) || !adam.p) return QHEA_EINVAL;
            fp.ld = mi.sh.fast_ld;
            fp.nbk = model_fuse_blocks(mi, M.L);
            fp.L = M.L.zL; fp.runs = mi.sh.runs;
            fp.rec = ws + M.L.off_rec; fp.srec = M.L.srecords ? ws + M.L.off_srec : nullptr;
            fp.gmap = reinterpret_cast<double*>(ws + M.L.off_gmap);
            rb.nb_w = (int)(mi.sh.blk / fp.ld / fp.nbk);        // one reduce block per circuit block (n = 2, ld = 1: per two)
        }
        if (dpx && !dp_blocks_ok(rb.total())) return QHEA_EUNSUPPORTED;
        if (!records_ready) {
            rc = launch_prep_zyz(mi.n, mi.sh, params + mi.off_ans, ws, M.L, st, R, ms);
            if (rc != QHEA_OK) return rc;
        }
        rc = launch_zyz_backward(k, mi.n, mi.sh, batch, M.L, ws, AngleSrc{nullptr, enc}, desc->ham_offset, desc->ham_coeff, ham_diag,
                                 desc->ham_pauli, nullptr, nullptr, v.y, bias, v.inv_bt, pr, gx, partial, st, R, ms,
                                 mlr ? mlr->mrec : nullptr);
        if (rc != QHEA_OK) return rc;
        return launch_reduce_model(rb, st, mi, M.L.nwaves, partial, params, v, enc, gx, pr, adam, ws,
                                   reinterpret_cast<const double*>(ws + M.L.off_gmap), fp, dpx, R, ms, mlr);
    }
    if (R != 1) return QHEA_EUNSUPPORTED;                       // (the ensemble entry point never asks: R-sequential calls there)
    if (records_ready || records_for_next) return QHEA_EINVAL;
    if (dpx && !dp_blocks_ok(rb.total())) return QHEA_EUNSUPPORTED;
    rc = launch_prep_model(desc, mi, batch, v.branch, v.trunk, params, reinterpret_cast<double4*>(ws + M.L.off_U),
                           reinterpret_cast<double2*>(ws + M.L.off_cs), ws, st);
    if (rc == QHEA_OK)
        rc = launch_table_backward(k, mi.n, mi.sh, batch, M.L, ws, desc->ham_offset, desc->ham_coeff, ham_diag, desc->ham_pauli,
                                   nullptr, nullptr, v.y, bias, v.inv_bt, pr, gx, partial, st);
    if (rc != QHEA_OK) return rc;
    return launch_reduce_model(rb, st, mi, M.L.nwaves, partial, params, v, enc, gx, pr, adam, ws, nullptr, FusePrep{}, dpx);
}

// The steps of qhea_model_train_steps and of qhea_model_dp_train_steps (dx: its exchange, step i's number first_seq + i); the
// arguments have been checked.
// Between two steps of equal batch size (same workspace layout) on a block-unrolled shape the first one's reduce kernel
// writes the second one's layer records: nobody else can touch the parameters in between, so the prep launch is dropped.
static int model_steps(const qhea_model_desc* desc, const ModelInfo& mi, const double* ham_diag, double lr, const TrainCall& c,
                       DpX* dx = nullptr, int64_t first_seq = 0) {
    bool ready = false;
    for (int64_t i = 0; i < c.n_steps; ++i) {
        const StepView v = step_view(c, i, *desc);
        bool next = false;
        if (i + 1 < c.n_steps && c.row_begin[i + 2] - c.row_begin[i + 1] == v.nb)
            next = model_fuse_eligible(mi, make_model_layout(mi, v.nb).L);
        if (dx) dx->seq = (unsigned long long)(first_seq + i);
        const int rc = model_loss_grad_impl(desc, v, c.params, ham_diag, nullptr, c.workspace, c.workspace_bytes, c.stream,
                                            adam_step(c, i, lr).adam, ready, next, dx);
        if (rc != QHEA_OK) return rc;
        ready = next;
    }
    return QHEA_OK;
}

// the optimizer state of a one-step call (qhea_model_train_step, qhea_adam_step) as a call record: step 0 is Adam step `step`
static TrainCall optimizer_call(double* params, double* exp_avg, double* exp_avg_sq, int64_t step, double beta1, double beta2,
                                double eps, double weight_decay) {
    TrainCall c{};
    c.params = params; c.exp_avg = exp_avg; c.exp_avg_sq = exp_avg_sq; c.first_step = step;
    c.beta1 = beta1; c.beta2 = beta2; c.eps = eps; c.weight_decay = weight_decay;
    return c;
}

int qhea_model_forward(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                       const double* params, const double* ham_diag, double* pred, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return model_forward_impl(desc, batch, branch, trunk, params, ham_diag, pred, workspace, workspace_bytes, stream, false);
}

int qhea_model_forward_chunks(const qhea_model_desc* desc, int64_t n_chunks, const int64_t* row_begin,
                              const double* branch, const double* trunk, const double* params, const double* ham_diag,
                              double* pred, void* workspace, size_t workspace_bytes, void* stream) {
    if (!desc || n_chunks < 0 || !row_begin || !branch || !params || !pred) return QHEA_EINVAL;
    ModelInfo mi;
    const int rc0 = model_info(desc, mi);
    if (rc0 != QHEA_OK) return rc0;
    const bool has_trunk = desc->model == QHEA_MODEL_QUANONET;
    if (has_trunk && !trunk) return QHEA_EINVAL;
    if (schedule_max_batch(n_chunks, row_begin) < 0) return QHEA_EINVAL;
    // the layer records depend on the parameters alone: one prep launch serves every chunk whose workspace layout keeps
    // them where the last prep put them (chunks of equal size; a shorter last chunk gets its own)
    Layout last{};
    bool have = false;                  // `last`: where a prep_zyz launch of this call left the records
    for (int64_t i = 0; i < n_chunks; ++i) {
        const int64_t r0 = row_begin[i], nb = row_begin[i + 1] - r0;
        const Layout L = make_model_layout(mi, nb).L;
        const bool zyz = zyz_family(fwd_kernel_for(L.in, CallTraits{desc->ham_pauli}));
        const bool ready = have && zyz && L.off_rec == last.off_rec && L.off_srec == last.off_srec &&
                           L.off_gmap == last.off_gmap && L.srecords == last.srecords && L.zL == last.zL;
        const int rc = model_forward_impl(desc, nb, branch + r0 * desc->branch_in,
                                          has_trunk ? trunk + r0 * desc->trunk_in : nullptr, params, ham_diag, pred + r0,
                                          workspace, workspace_bytes, stream, ready);
        if (rc != QHEA_OK) return rc;
        if (!ready) { last = L; have = zyz; }
    }
    return QHEA_OK;
}

int qhea_model_loss_grad(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                         const double* y, const double* params, const double* ham_diag, double inv_batch_total,
                         double* grad, double* pred, void* workspace, size_t workspace_bytes, void* stream) {
    return model_loss_grad_impl(desc, StepView{0, batch, branch, trunk, y, grad, inv_batch_total}, params, ham_diag, pred,
                                workspace, workspace_bytes, stream, AdamArgs{});
}

int qhea_model_train_step(const qhea_model_desc* desc, int64_t batch, const double* branch, const double* trunk,
                          const double* y, double* params, const double* ham_diag, double inv_batch_total,
                          double* grad, double* pred, double* exp_avg, double* exp_avg_sq, int64_t step, double lr,
                          double beta1, double beta2, double eps, double weight_decay, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (step < 1 || !params || !exp_avg || !exp_avg_sq || batch <= 0) return QHEA_EINVAL;
    const TrainCall opt = optimizer_call(params, exp_avg, exp_avg_sq, step, beta1, beta2, eps, weight_decay);
    return model_loss_grad_impl(desc, StepView{0, batch, branch, trunk, y, grad, inv_batch_total}, params, ham_diag, pred,
                                workspace, workspace_bytes, stream, adam_step(opt, 0, lr).adam);
}

int qhea_model_train_steps(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                           const double* branch, const double* trunk, const double* y, double* params,
                           const double* ham_diag, const double* inv_batch_total, double* grad, int64_t grad_stride,
                           double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                           double beta2, double eps, double weight_decay, void* workspace, size_t workspace_bytes,
                           void* stream) {
    if (!desc || n_steps < 0 || !row_begin || !inv_batch_total || !branch || !y || !grad || first_step < 1)
        return QHEA_EINVAL;
    ModelInfo mi;
    const int rc0 = model_info(desc, mi);
    if (rc0 != QHEA_OK) return rc0;
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    if (call_max_batch(call, mi.P, *desc) < 0) return QHEA_EINVAL;
    return model_steps(desc, mi, ham_diag, lr, call);
}

int qhea_model_dp_train_steps(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin,
                              const double* branch, const double* trunk, const double* y, double* params,
                              const double* ham_diag, const double* inv_batch_total, double* grad, int64_t grad_stride,
                              double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                              double beta2, double eps, double weight_decay, int rank, int world, void* const* buffers,
                              int64_t dp_values, int64_t first_seq, double timeout_ms, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!desc || n_steps < 0 || !row_begin || !inv_batch_total || !branch || !y || !grad || first_step < 1)
        return QHEA_EINVAL;
    if (world < 2 || world > QHEA_DP_MAX_RANKS || rank < 0 || rank >= world || !buffers || first_seq < 1 || !(timeout_ms > 0.0))
        return QHEA_EINVAL;
    ModelInfo mi;
    const int rc0 = model_info(desc, mi);
    if (rc0 != QHEA_OK) return rc0;
    if (grad_stride < mi.P + 2 || dp_values < mi.P + 2) return QHEA_EINVAL;
    if (desc->model == QHEA_MODEL_QUANONET && !trunk) return QHEA_EINVAL;
    if (!params || !exp_avg || !exp_avg_sq) return QHEA_EINVAL;
    DpX dx{};
    for (int r = 0; r < world; ++r) {
        if (!buffers[r]) return QHEA_EINVAL;
        dx.bufs[r] = static_cast<char*>(buffers[r]);
    }
    dx.rank = rank; dx.world = world; dx.npad = dp_padded((long)dp_values);
    dx.timeout_ticks = (long long)(timeout_ms * 1e5);           // wall_clock64: 100 MHz
    // every step must be launchable BEFORE the first one is (a rank that stops half-way would leave its peers waiting):
    // no empty shard, and a reduce grid that fits the device and the exchange buffers' block flags
    // (its own schedule rule: an empty shard is well-formed, and refused as unsupported)
    for (int64_t i = 0; i < n_steps; ++i) {
        if (row_begin[i] < 0 || row_begin[i + 1] < row_begin[i]) return QHEA_EINVAL;
        if (row_begin[i + 1] == row_begin[i]) return QHEA_EUNSUPPORTED;
    }
    if (!dp_blocks_ok(red_blocks(mi.n, mi.sh.blk, mi.sh.E, mi.trainable).total())) return QHEA_EUNSUPPORTED;   // (the fused reduce uses fewer)
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    return model_steps(desc, mi, ham_diag, lr, call, &dx, first_seq);
}

// Ensembles and sweeps whose every step runs the ZYZ kernels (members_train_steps): one grid per kernel and step.  R = 1 runs
// the single-model kernels on member 0's descriptor; R > 1 the member kernels, which read every member's read-out, scale and
// learning rate from its MemberRec.  The arguments and the slice size have been checked by the caller.
static int members_zyz_grid(const qhea_model_desc* desc, const ModelInfo& mi, int64_t n_models,
                            const qhea_member_hparams* members, int64_t member_step, const double* diag0, int64_t diag_stride,
                            size_t slice, const TrainCall& c) {
    hipStream_t st = c.st();
    char* ws = c.ws();
    // The launch descriptor only chooses the kernels: a member that reads out X or Y gives the whole launch the kernels of an
    // X / Y model (the split-layout chains are Z-only).
    const qhea_member_hparams& h0 = members[0];
    qhea_model_desc dl = member_desc(*desc, h0);
    if (n_models > 1) {
        for (int64_t m = 0; m < n_models; ++m)
            if (members[m * member_step].ham_pauli != QHEA_PAULI_Z) dl.ham_pauli = QHEA_PAULI_X;
        const int rc = fill_member_recs<MemberFill>(n_models, ws, slice, diag0, diag_stride, st,
                                                    [&](MemberFill& f, int i, int64_t m) { f.h[i] = members[m * member_step]; });
        if (rc != QHEA_OK) return rc;
    }
    const MemberStride ms{(long)c.row_begin[c.n_steps] /* rows per member */, (long)mi.P, (long)(c.n_steps * c.grad_stride),
                          (long)slice};
    bool ready = false;
    for (int64_t i = 0; i < c.n_steps; ++i) {
        const StepView v = step_view(c, i, *desc);
        bool next = false;
        if (i + 1 < c.n_steps && c.row_begin[i + 2] - c.row_begin[i + 1] == v.nb)
            next = model_fuse_eligible(mi, make_model_layout(mi, v.nb, n_models * v.nb).L);
        const AdamStep as = adam_step(c, i, h0.lr);
        const MemberLr mlr{ws + kMemberRecOffset, as.bc1};
        const int rc = model_loss_grad_impl(&dl, v, c.params, diag0, nullptr, ws, slice, c.stream, as.adam, ready, next, nullptr,
                                            (int)n_models, ms, n_models > 1 ? &mlr : nullptr);
        if (rc != QHEA_OK) return rc;
        ready = next;
    }
    return QHEA_OK;
}

// ---- depth sweeps (qhea_model_depth_sweep_train_steps), and the member grid of ensembles and sweeps at n >= 10 ----
// The members' descriptors: every field but the depths (QuanONet net[0] / net[2], HEAQNN net[0]) equal to member 0's, each one
// valid on its own (its ham_* and scale fields are not used: read with a Z read-out).  env: the descriptor with the largest
// depths of every run -- its shape bounds every member's E, blk and P, and sizes the slices and the grids.
struct DepthSet {
    qhea_model_desc env;
    ModelInfo env_mi;
    int64_t pmax = 0;
    int c_max[2] = {0, 0};
    DepthRed dr{};
};
// member m's block counts of run 0 / run 1 of the launch's run table: QuanONet trunk (net[2] x net[3]) then branch
// (net[0] x net[1]); HEAQNN net[0] x net[1] and an empty run
static void depth_counts(const qhea_model_desc& d, int32_t (&c)[2]) {
    const bool qn = d.model == QHEA_MODEL_QUANONET;
    c[0] = qn ? d.net[2] : d.net[0];
    c[1] = qn ? d.net[0] : 0;
}
static DepthRed depth_red(const qhea_model_desc& d) {
    const bool qn = d.model == QHEA_MODEL_QUANONET;
    return DepthRed{qn ? 1 : 0, d.trainable_freq != 0 ? 1 : 0, qn ? d.net[3] : d.net[1], qn ? d.net[1] : 0};
}
// Member d (mi: its model_info) joins the set: the run lengths, the largest counts and P.  QHEA_EUNSUPPORTED where the member
// kernels' parameter layout (depth_map) is not the model's.
static int depth_set_add(DepthSet& ds, const qhea_model_desc& d, const ModelInfo& mi) {
    int32_t c[2];
    depth_counts(d, c);
    ds.dr = depth_red(d);
    if (depth_map(mi.n, ds.dr.quanonet != 0, mi.trainable, c[0], c[1], ds.dr.ld0, ds.dr.ld1).P != mi.P) return QHEA_EUNSUPPORTED;
    if (mi.P > ds.pmax) ds.pmax = mi.P;
    if (c[0] > ds.c_max[0]) ds.c_max[0] = c[0];
    if (c[1] > ds.c_max[1]) ds.c_max[1] = c[1];
    return QHEA_OK;
}
static int depth_set(const qhea_model_desc* descs, int64_t R, DepthSet& ds) {
    if (!descs || R < 1 || R > 65535) return QHEA_EINVAL;
    const qhea_model_desc& d0 = descs[0];
    const bool qn = d0.model == QHEA_MODEL_QUANONET;
    ds.env = d0;
    ds.env.ham_pauli = QHEA_PAULI_Z;
    for (int64_t m = 0; m < R; ++m) {
        const qhea_model_desc& d = descs[m];
        if (d.model != d0.model || d.n_qubits != d0.n_qubits || d.branch_in != d0.branch_in || d.trunk_in != d0.trunk_in ||
            d.trainable_freq != d0.trainable_freq || d.net[1] != d0.net[1] || d.net[3] != d0.net[3] ||
            (!qn && d.net[2] != d0.net[2]))
            return QHEA_EINVAL;
        qhea_model_desc dz = d;
        dz.ham_pauli = QHEA_PAULI_Z;
        ModelInfo mi;
        int rc = model_info(&dz, mi);
        if (rc == QHEA_OK) rc = depth_set_add(ds, d, mi);
        if (rc != QHEA_OK) return rc;
    }
    if (qn) { ds.env.net[2] = ds.c_max[0]; ds.env.net[0] = ds.c_max[1]; }
    else ds.env.net[0] = ds.c_max[0];
    return model_info(&ds.env, ds.env_mi);
}
// One member's slice for `batch` rows (the largest member's shape): header (MemberRec at kMemberRecOffset), gate table, (cos, sin)
// table, partial rows of the backward kernel, grad_x, predictions -- the first-generation single-model layout under
// QHEA_BWD_PACKED (n >= 10: the workgroup-resident kernel's, one partial row per sample)
struct DepthLayout { size_t off_U, off_cs, off_part, off_gx, off_pred, total; long nwaves; };
static DepthLayout depth_layout(const ModelInfo& env, int64_t B) {
    DepthLayout L{};
    const int n = env.n, spw = 64 >> lane_bits(n);
    L.nwaves = lds_supported(n) ? (long)B : (((B + spw - 1) / spw + kWaves - 1) / kWaves) * kWaves;
    const TableLayout t = table_layout(env, B);
    L.off_U = t.off_gates; L.off_cs = t.off_cs;
    size_t p = t.end;
    L.off_part = p; p = align256(p + (size_t)L.nwaves * env.sh.blk * padded_3n(n) * sizeof(double));
    L.off_gx = p;   p = align256(p + (size_t)B * env.sh.E * sizeof(double));
    L.off_pred = p; p = align256(p + (size_t)B * sizeof(double));
    L.total = p;
    return L;
}
static size_t depth_slice_bytes(const DepthSet& ds, int64_t batch) { return depth_layout(ds.env_mi, batch).total; }

// One grid per kernel and step for R members of one model kind, n and run lengths whose block counts may differ (ds: their
// envelope, DepthSet): depth sweeps, and ensembles / sweeps at n >= 10, whose members share one shape.  Member m's block counts
// are those of descs[m * desc_step] (desc_step 0: one descriptor for all), its hyper-parameters members[m * member_step]
// (member_step 0: one record for all), its diagonal Hamiltonian diag0 + m * diag_stride.  n <= 9: the packed backward kernel's
// member form; n >= 10: the workgroup-resident one's.  The arguments and the slice size (>= depth_slice_bytes for every batch
// of the schedule) have been checked by the caller.
static int depth_grid_steps(const DepthSet& ds, int64_t n_models, const qhea_model_desc* descs, int64_t desc_step,
                            const qhea_member_hparams* members, int64_t member_step, const double* diag0, int64_t diag_stride,
                            size_t slice, const TrainCall& c) {
    const ModelInfo& env = ds.env_mi;
    const bool qn = ds.env.model == QHEA_MODEL_QUANONET;
    char* ws = c.ws();
    hipStream_t st = c.st();
    // One grid per kernel and step, member = blockIdx.y: every member's read-out, scale, learning rate and block counts reach
    // its MemberRec first
    const int rc = fill_member_recs<MemberFillDepth>(n_models, ws, slice, diag0, diag_stride, st,
                                                     [&](MemberFillDepth& f, int i, int64_t m) {
        f.h[i] = members[m * member_step];
        depth_counts(descs[m * desc_step], f.depth[i]);
    });
    if (rc != QHEA_OK) return rc;
    // the reduce grid: the most blocks any member's roles need (ansatz blocks, frequency blocks, the sse / bias block)
    const int n = env.n;
    int red_grid = 0;
    for (int64_t m = 0; m < n_models; ++m) {
        int32_t cnt[2];
        depth_counts(descs[m * desc_step], cnt);
        const DepthMap d = depth_map(n, qn, ds.dr.trainable != 0, cnt[0], cnt[1], ds.dr.ld0, ds.dr.ld1);
        red_grid = std::max(red_grid, red_blocks(n, d.blk, d.E, ds.dr.trainable != 0).total());
    }
    const Runs runs = two_runs(n, ds.dr.ld0, ds.dr.ld1);
    const MemberStride ms{(long)c.row_begin[c.n_steps] /* rows per member */, (long)ds.pmax, (long)(c.n_steps * c.grad_stride),
                          (long)slice};
    const char* mrec = ws + kMemberRecOffset;
    const GradMap gm = grad_map(env);
    for (int64_t i = 0; i < c.n_steps; ++i) {
        const StepView v = step_view(c, i, ds.env);
        const DepthLayout L = depth_layout(env, v.nb);
        const EncDesc enc = make_enc(&ds.env, env, v.branch, v.trunk, c.params);
        const long prep_total = (env.sh.blk + 2) * n + v.nb * env.sh.E;
        hipLaunchKernelGGL(prep_model_depth_kernel, dim3((unsigned)((prep_total + 255) / 256), (unsigned)n_models), dim3(256), 0, st,
                           n, ds.dr, (const double*)c.params, reinterpret_cast<double4*>(ws + L.off_U), (long)v.nb, enc,
                           reinterpret_cast<double2*>(ws + L.off_cs), reinterpret_cast<WorkspaceHeader*>(ws), mrec, ms);
        if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
        double* gx = reinterpret_cast<double*>(ws + L.off_gx);
        double* pr = reinterpret_cast<double*>(ws + L.off_pred);
        double* partial = reinterpret_cast<double*>(ws + L.off_part);
        const BwdArgs ba{runs, (long)v.nb, (int)env.sh.E, (int)env.sh.blk, reinterpret_cast<const double2*>(ws + L.off_cs),
                         ws + L.off_U, 0, 0.0, 0.0, nullptr, nullptr, nullptr, v.y, qn ? c.params : nullptr,
                         v.inv_bt, pr, gx, partial, QHEA_PAULI_Z, 0, dense_bit(n_models * L.nwaves),
                         nullptr};
        const dim3 grid((unsigned)(L.nwaves / kWaves), (unsigned)n_models);
        profile_begin(st);
        if (lds_supported(n)) {                          // one workgroup per (sample, member)
            const int rcl = launch_lds_bwd_depth(n, dim3((unsigned)v.nb, (unsigned)n_models), st, ba, DepthArgs{mrec, ms});
            if (rcl != QHEA_OK) return rcl;
        } else switch (n) {
#define QHEA_CASE(NN) case NN: launch_bwd_depth_##NN(grid, st, ba, mrec, ms); break;
            QHEA_FOR_EACH_N(QHEA_CASE)
#undef QHEA_CASE
            default: return QHEA_EUNSUPPORTED;
        }
        profile_end(st);
        if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
        const AdamStep as = adam_step(c, i, members[0].lr);
        hipLaunchKernelGGL((reduce_model_kernel<false, false, true, DepthRed>), dim3((unsigned)red_grid, (unsigned)n_models),
                           dim3(kRedThreads), 0, st, n, (int)env.sh.blk, padded_3n(n), L.nwaves, (const double*)partial,
                           (const double*)c.params, (long)v.nb, (int)env.sh.E, enc, (const double*)gx, (const double*)pr, v.y,
                           v.inv_bt, gm, 0, 0, v.grad, as.adam,
                           reinterpret_cast<const WorkspaceHeader*>(ws), (const double*)nullptr, FusePrep{}, DpX{}, ms,
                           MemberLr{mrec, as.bc1}, ds.dr);
        if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    }
    return QHEA_OK;
}

// Ensembles and sweeps at n >= 10 (members_train_steps, R > 1): a depth sweep whose members all have the descriptor's block
// counts.  Its slices are the ensemble's (the single-model layout, which depth_layout reproduces).  QHEA_EUNSUPPORTED before
// any launch when the shape has no depth-sweep form.
static int members_lds_grid(const qhea_model_desc* desc, const ModelInfo& mi, int64_t n_models,
                            const qhea_member_hparams* members, int64_t member_step, const double* diag0, int64_t diag_stride,
                            size_t slice, const TrainCall& c) {
    DepthSet ds;
    ds.env = *desc;
    ds.env.ham_pauli = QHEA_PAULI_Z;
    if (model_info(&ds.env, ds.env_mi) != QHEA_OK || depth_set_add(ds, *desc, mi) != QHEA_OK) return QHEA_EUNSUPPORTED;
    for (int64_t i = 0; i < c.n_steps; ++i)
        if (depth_slice_bytes(ds, c.row_begin[i + 1] - c.row_begin[i]) > slice) return QHEA_EUNSUPPORTED;
    return depth_grid_steps(ds, n_models, desc, 0, members, member_step, diag0, diag_stride, slice, c);
}

// qhea_model_ensemble_train_steps and qhea_model_sweep_train_steps: R members of one shape, member m with hyper-parameters
// members[m * member_step] (member_step 0: one record for all) and diagonal Hamiltonian diag0 + m * diag_stride (diag0 ==
// nullptr: none).  The arguments have been checked by the caller.
static int members_train_steps(const qhea_model_desc* desc, const ModelInfo& mi, int64_t n_models,
                               const qhea_member_hparams* members, int64_t member_step, const double* diag0,
                               int64_t diag_stride, const TrainCall& c) {
    // one slice per member, sized for every batch size of the schedule; one launch per kernel where every step runs the ZYZ
    // kernels or (n >= 10) the workgroup-resident ones, R consecutive single-model calls otherwise (n = 6..9)
    size_t slice = 0;
    bool grid = true;
    for (int64_t i = 0; i < c.n_steps; ++i) {
        const int64_t nb = c.row_begin[i + 1] - c.row_begin[i];
        const size_t b = ensemble_slice_bytes(mi, n_models, nb);
        if (b > slice) slice = b;
        grid = grid && n_models <= 65535 && ensemble_grid(mi, n_models, nb);      // (gridDim.y)
    }
    if (!c.workspace || c.workspace_bytes / (size_t)n_models < slice) return QHEA_EWORKSPACE;
    if (grid) return members_zyz_grid(desc, mi, n_models, members, member_step, diag0, diag_stride, slice, c);
    if (n_models > 1 && lds_supported(mi.n)) {
        const int rc = members_lds_grid(desc, mi, n_models, members, member_step, diag0, diag_stride, slice, c);
        if (rc != QHEA_EUNSUPPORTED) return rc;                   // (unsupported: found before anything was launched)
    }
    const int64_t rows = c.row_begin[c.n_steps];                    // rows per member
    for (int64_t m = 0; m < n_models; ++m) {
        const qhea_member_hparams& h = members[m * member_step];
        const qhea_model_desc dm = member_desc(*desc, h);
        TrainCall cm = c;                                           // member m's arrays and workspace slice
        cm.branch += m * rows * desc->branch_in;
        if (cm.trunk) cm.trunk += m * rows * desc->trunk_in;
        cm.y += m * rows;
        cm.params += m * mi.P; cm.exp_avg += m * mi.P; cm.exp_avg_sq += m * mi.P;
        cm.grad += m * c.n_steps * c.grad_stride;
        cm.workspace = c.ws() + m * slice; cm.workspace_bytes = slice;
        const int rc = model_steps(&dm, mi, diag0 ? diag0 + m * diag_stride : nullptr, h.lr, cm);
        if (rc != QHEA_OK) return rc;
        if (m > 0) {
            hipLaunchKernelGGL(status_fold_kernel, dim3(1), dim3(64), 0, c.st(), reinterpret_cast<WorkspaceHeader*>(c.workspace),
                               reinterpret_cast<WorkspaceHeader*>(cm.workspace));
            if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
        }
    }
    return QHEA_OK;
}

size_t qhea_model_ensemble_workspace_bytes(const qhea_model_desc* desc, int64_t n_models, int64_t batch) {
    ModelInfo mi;
    if (model_info(desc, mi) != QHEA_OK || n_models < 1 || batch < 0) return 0;
    return (size_t)n_models * ensemble_slice_bytes(mi, n_models, batch);
}

int qhea_model_ensemble_train_steps(const qhea_model_desc* desc, int64_t n_models, int64_t n_steps, const int64_t* row_begin,
                                    const double* branch, const double* trunk, const double* y, double* params,
                                    const double* ham_diag, const double* inv_batch_total, double* grad, int64_t grad_stride,
                                    double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                                    double beta2, double eps, double weight_decay, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    if (!desc || n_models < 1 || n_steps < 1 || !row_begin || !inv_batch_total || !branch || !y || !grad || first_step < 1)
        return QHEA_EINVAL;
    ModelInfo mi;
    const int rc0 = model_info(desc, mi);
    if (rc0 != QHEA_OK) return rc0;
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    if (!pauli_ok(desc->ham_pauli, ham_diag) || call_max_batch(call, mi.P, *desc) < 0) return QHEA_EINVAL;
    // a sweep whose members all share the descriptor's read-out and scale and `lr` (one shared ham_diag)
    const qhea_member_hparams uni{desc->scale_coeff, desc->ham_offset, desc->ham_coeff, lr, desc->ham_pauli, 0};
    return members_train_steps(desc, mi, n_models, &uni, 0, ham_diag, 0, call);
}

size_t qhea_model_sweep_workspace_bytes(const qhea_model_desc* desc, int64_t n_models, int64_t batch) {
    return qhea_model_ensemble_workspace_bytes(desc, n_models, batch);      // (the MemberRecs live in the slices' headers)
}

int qhea_model_sweep_train_steps(const qhea_model_desc* desc, int64_t n_models, const qhea_member_hparams* members,
                                 const double* ham_diag, int64_t n_steps, const int64_t* row_begin, const double* branch,
                                 const double* trunk, const double* y, double* params, const double* inv_batch_total,
                                 double* grad, int64_t grad_stride, double* exp_avg, double* exp_avg_sq, int64_t first_step,
                                 double beta1, double beta2, double eps, double weight_decay, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!desc || n_models < 1 || !members || n_steps < 1 || !row_begin || !inv_batch_total || !branch || !y || !grad ||
        first_step < 1)
        return QHEA_EINVAL;
    if (!member_records_ok(members, n_models, ham_diag)) return QHEA_EINVAL;
    // the shape (and everything model_info checks) is the descriptor's; its scale and Hamiltonian fields are not used
    const qhea_model_desc d0 = member_desc(*desc, members[0]);
    ModelInfo mi;
    const int rc0 = model_info(&d0, mi);
    if (rc0 != QHEA_OK) return rc0;
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    if (call_max_batch(call, mi.P, d0) < 0) return QHEA_EINVAL;
    return members_train_steps(&d0, mi, n_models, members, 1, ham_diag, (int64_t)1 << mi.n, call);
}

size_t qhea_model_depth_sweep_workspace_bytes(const qhea_model_desc* descs, int64_t n_models, int64_t batch) {
    DepthSet ds;
    if (depth_set(descs, n_models, ds) != QHEA_OK || batch < 0) return 0;
    return (size_t)n_models * depth_slice_bytes(ds, batch);
}

int qhea_model_depth_sweep_train_steps(const qhea_model_desc* descs, int64_t n_models, const qhea_member_hparams* members,
                                       const double* ham_diag, int64_t n_steps, const int64_t* row_begin, const double* branch,
                                       const double* trunk, const double* y, double* params, const double* inv_batch_total,
                                       double* grad, int64_t grad_stride, double* exp_avg, double* exp_avg_sq,
                                       int64_t first_step, double beta1, double beta2, double eps, double weight_decay,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!descs || n_models < 1 || !members || n_steps < 1 || !row_begin || !inv_batch_total || !branch || !y || !grad ||
        first_step < 1)
        return QHEA_EINVAL;
    if (!member_records_ok(members, n_models, ham_diag)) return QHEA_EINVAL;
    DepthSet ds;
    const int rc0 = depth_set(descs, n_models, ds);
    if (rc0 != QHEA_OK) return rc0;
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    if (call_max_batch(call, ds.pmax, ds.env) < 0) return QHEA_EINVAL;
    size_t slice = 0;
    for (int64_t i = 0; i < n_steps; ++i) {
        const size_t b = depth_slice_bytes(ds, row_begin[i + 1] - row_begin[i]);
        if (b > slice) slice = b;
    }
    if (!workspace || slice == 0 || workspace_bytes < (size_t)n_models * slice) return QHEA_EWORKSPACE;
    return depth_grid_steps(ds, n_models, descs, 1, members, 1, ham_diag, (int64_t)1 << ds.env_mi.n, slice, call);
}

// ---- qubit sweeps (qhea_model_qubit_sweep_train_steps) ----
// The members' descriptors: every field but n_qubits and the depths equal to member 0's, each one valid on its own (its ham_*
// and scale fields are not used: read with a Z read-out).  Members with n <= 9 run the wave-resident kernels, members with
// n >= 10 the workgroup-resident ones (hea_lds.hip); every member shares the sweep's launches.
struct QubitMember {
    ModelInfo mi;
    int32_t c[2];               // block counts of run 0 / run 1 (MemberRec::depth)
    DepthMap d;
    bool wave;                  // n <= 9
    double cost;                // length of the backward chain of one sample group (sub-layers x gates x amplitudes per lane;
                                // n >= 10: per thread of the sample's workgroup, up to a constant)
};
struct QubitSet {
    std::vector<QubitMember> mem;
    int64_t pmax = 0;
    int nmax = 0;
    DepthRed dr{};
};
static int qubit_set(const qhea_model_desc* descs, int64_t R, QubitSet& qs) {
    if (!descs || R < 1 || R > 65535) return QHEA_EINVAL;
    const qhea_model_desc& d0 = descs[0];
    const bool qn = d0.model == QHEA_MODEL_QUANONET;
    qs.mem.resize((size_t)R);
    for (int64_t m = 0; m < R; ++m) {
        const qhea_model_desc& d = descs[m];
        if (d.model != d0.model || d.branch_in != d0.branch_in || d.trunk_in != d0.trunk_in ||
            d.trainable_freq != d0.trainable_freq || d.net[1] != d0.net[1] || d.net[3] != d0.net[3] ||
            (!qn && d.net[2] != d0.net[2]))
            return QHEA_EINVAL;
        qhea_model_desc dz = d;
        dz.ham_pauli = QHEA_PAULI_Z;
        QubitMember& q = qs.mem[(size_t)m];
        const int rc = model_info(&dz, q.mi);
        if (rc != QHEA_OK) return rc;
        const int n = q.mi.n;
        depth_counts(d, q.c);
        qs.dr = depth_red(d);
        q.d = depth_map(n, qn, q.mi.trainable, q.c[0], q.c[1], qs.dr.ld0, qs.dr.ld1);
        if (q.d.P != q.mi.P) return QHEA_EUNSUPPORTED;
        q.wave = !lds_supported(n);
        if (q.wave && !qs_built(n)) return QHEA_EUNSUPPORTED;      // (development builds)
        q.cost = (double)q.d.blk * n * (double)(1 << (n - lane_bits(n)));
        if (q.mi.P > qs.pmax) qs.pmax = q.mi.P;
        if (n > qs.nmax) qs.nmax = n;
    }
    return QHEA_OK;
}
// Work lists for a schedule whose largest batch is Bmax: per register class its members' (member, sample group) entries, the
// longest chain first (a short batch's launch skips the groups past its last sample); per n = 7..9 its members (member, 0);
// per n = 10..12 its members (member, 0), the longest chain first; then every member's reduce roles (ansatz blocks, frequency
// blocks, the sse / bias block) as (member, role).
constexpr int kQsLdsLo = 10, kQsLdsHi = 12;     // workgroup-resident members: one launch per n, member = entry blockIdx.y
struct QubitPlan {
    std::vector<int2> e;
    int cls_begin[kQsClasses] = {0, 0}, cls_count[kQsClasses] = {0, 0};
    int own_begin[kQsOwnHi - kQsOwnLo + 1] = {0, 0, 0}, own_count[kQsOwnHi - kQsOwnLo + 1] = {0, 0, 0};   // n = 7..9: (member, 0)
    int lds_begin[kQsLdsHi - kQsLdsLo + 1] = {0, 0, 0}, lds_count[kQsLdsHi - kQsLdsLo + 1] = {0, 0, 0};   // n = 10..12: (member, 0)
    int red_begin = 0, red_count = 0;
    int per = 1;                // entries per slice
    size_t list_bytes = 0;
};
static int red_roles(const QubitMember& q, bool trainable) {
    return red_blocks(q.mi.n, q.d.blk, q.d.E, trainable).total();
}
static void qubit_plan(const QubitSet& qs, int64_t Bmax, QubitPlan& P) {
    const int64_t R = (int64_t)qs.mem.size();
    for (int c = 0; c < kQsClasses; ++c) {
        std::vector<int> ms;
        for (int64_t m = 0; m < R; ++m)
            if (qs.mem[m].wave && qs_class_of(qs.mem[m].mi.n) == c) ms.push_back((int)m);
        std::stable_sort(ms.begin(), ms.end(), [&](int a, int b) { return qs.mem[a].cost > qs.mem[b].cost; });
        P.cls_begin[c] = (int)P.e.size();
        for (int m : ms) {
            const long groups = qs_nwaves(qs.mem[m].mi.n, Bmax) / kWaves;
            for (long g = 0; g < groups; ++g) P.e.push_back(make_int2(m, (int)g));
        }
        P.cls_count[c] = (int)P.e.size() - P.cls_begin[c];
    }
    for (int n = kQsOwnLo; n <= kQsOwnHi; ++n) {
        P.own_begin[n - kQsOwnLo] = (int)P.e.size();
        for (int64_t m = 0; m < R; ++m)
            if (qs.mem[m].wave && qs.mem[m].mi.n == n) P.e.push_back(make_int2((int)m, 0));
        P.own_count[n - kQsOwnLo] = (int)P.e.size() - P.own_begin[n - kQsOwnLo];
    }
    for (int n = kQsLdsLo; n <= kQsLdsHi; ++n) {
        std::vector<int> ms;
        for (int64_t m = 0; m < R; ++m)
            if (qs.mem[m].mi.n == n) ms.push_back((int)m);
        std::stable_sort(ms.begin(), ms.end(), [&](int a, int b) { return qs.mem[a].cost > qs.mem[b].cost; });
        P.lds_begin[n - kQsLdsLo] = (int)P.e.size();
        for (int m : ms) P.e.push_back(make_int2(m, 0));
        P.lds_count[n - kQsLdsLo] = (int)P.e.size() - P.lds_begin[n - kQsLdsLo];
    }
    P.red_begin = (int)P.e.size();
    for (int64_t m = 0; m < R; ++m)
        for (int r = 0, nr = red_roles(qs.mem[m], qs.dr.trainable != 0); r < nr; ++r) P.e.push_back(make_int2((int)m, r));
    P.red_count = (int)P.e.size() - P.red_begin;
    P.per = (int)(((int64_t)P.e.size() + R - 1) / R);
    if (P.per < 1) P.per = 1;
    P.list_bytes = (size_t)P.per * sizeof(int2);
}
// One member's slice for `batch` rows: header (MemberRec at kMemberRecOffset), list region, then the depth sweep's regions --
// gate table, (cos, sin) table, partial rows of the member's backward kernel (qs_part_rows), grad_x, predictions -- each sized
// for the largest member's, so that every member's lie at the same offsets.
struct QubitLayout { size_t off_list, off_U, off_cs, off_part, off_gx, off_pred, total; };
static QubitLayout qubit_layout(const QubitSet& qs, int64_t B, size_t list_bytes) {
    size_t u = 0, e = 0, part = 0;
    for (const QubitMember& q : qs.mem) {
        const int n = q.mi.n;
        u = std::max(u, (size_t)(q.d.blk + 2) * n * kGateBytes);
        e = std::max(e, (size_t)q.d.E);
        part = std::max(part, (size_t)qs_part_rows(n, B) * q.d.blk * padded_3n(n) * sizeof(double));
    }
    QubitLayout L{};
    size_t p = kHeaderBytes;
    L.off_list = p; p = align256(p + list_bytes);
    L.off_U = p;    p = align256(p + u);
    L.off_cs = p;   p = align256(p + (size_t)B * e * sizeof(double2));
    L.off_part = p; p = align256(p + part);
    L.off_gx = p;   p = align256(p + (size_t)B * e * sizeof(double));
    L.off_pred = p; p = align256(p + (size_t)B * sizeof(double));
    L.total = p;
    return L;
}
static size_t qubit_slice_bytes(const QubitSet& qs, int64_t B, size_t list_bytes) { return qubit_layout(qs, B, list_bytes).total; }

size_t qhea_model_qubit_sweep_workspace_bytes(const qhea_model_desc* descs, int64_t n_models, int64_t batch) {
    QubitSet qs;
    if (qubit_set(descs, n_models, qs) != QHEA_OK || batch < 0) return 0;
    QubitPlan plan;
    qubit_plan(qs, batch, plan);
    return (size_t)n_models * qubit_slice_bytes(qs, batch, plan.list_bytes);
}

// The launches of a qubit sweep (plan: its work lists for the schedule's largest batch; d0: member 0's descriptor, whose
// input widths and frequency layout are every member's).  The arguments and the slice size have been checked by the caller.
static int qubit_grid_steps(const QubitSet& qs, const QubitPlan& plan, int64_t n_models, const qhea_model_desc& d0,
                            const qhea_member_hparams* members, const double* ham_diag, size_t slice, const TrainCall& c) {
    const bool qn = d0.model == QHEA_MODEL_QUANONET;
    hipStream_t st = c.st();
    char* ws = c.ws();
    // every member's read-out, scale, learning rate, block counts and n reach its MemberRec, the work lists the slices'
    // list regions
    const int rc = fill_member_recs<MemberFillQubit>(n_models, ws, slice, ham_diag, (int64_t)1 << qs.nmax, st,
                                                     [&](MemberFillQubit& f, int i, int64_t m) {
        f.h[i] = members[m];
        f.depth[i][0] = qs.mem[m].c[0]; f.depth[i][1] = qs.mem[m].c[1];
        f.nq[i] = qs.mem[m].mi.n;
    });
    if (rc != QHEA_OK) return rc;
    char* list0 = ws + kHeaderBytes;                             // (QubitLayout::off_list)
    for (int k0 = 0; k0 < (int)plan.e.size(); k0 += kWorkFill) {
        const int cnt = std::min<int>(kWorkFill, (int)plan.e.size() - k0);
        WorkFill f{};
        for (int i = 0; i < cnt; ++i) f.e[i] = plan.e[k0 + i];
        hipLaunchKernelGGL(work_fill_kernel, dim3(1), dim3(kWorkFill), 0, st, f, cnt, k0, list0, (long)slice, plan.per);
        if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    }
    const MemberStride ms{(long)c.row_begin[c.n_steps] /* rows per member */, (long)qs.pmax, (long)(c.n_steps * c.grad_stride),
                          (long)slice};
    const char* mrec = ws + kMemberRecOffset;
    QubitBwdArgs qa{};
    for (int n = 2; n <= 9; ++n) qa.runs[n - 2] = two_runs(n, qs.dr.ld0, qs.dr.ld1);
    const ModelInfo& mi0 = qs.mem[0].mi;
    const GradMap gm = grad_map(mi0);
    for (int64_t i = 0; i < c.n_steps; ++i) {
        const StepView v = step_view(c, i, d0);
        const QubitLayout L = qubit_layout(qs, v.nb, plan.list_bytes);
        const EncDesc enc = make_enc(&d0, mi0, v.branch, v.trunk, c.params);
        long prep_total = 0;
        for (const QubitMember& q : qs.mem)
            prep_total = std::max(prep_total, (long)(q.d.blk + 2) * q.mi.n + (long)v.nb * q.d.E);
        hipLaunchKernelGGL(prep_model_qubit_kernel, dim3((unsigned)((prep_total + 255) / 256), (unsigned)n_models), dim3(256), 0,
                           st, qs.dr, (const double*)c.params, reinterpret_cast<double4*>(ws + L.off_U), (long)v.nb, enc,
                           reinterpret_cast<double2*>(ws + L.off_cs), reinterpret_cast<WorkspaceHeader*>(ws), mrec, ms);
        if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
        double* gx = reinterpret_cast<double*>(ws + L.off_gx);
        double* pr = reinterpret_cast<double*>(ws + L.off_pred);
        double* partial = reinterpret_cast<double*>(ws + L.off_part);
        qa.B = v.nb; qa.inv_bt = v.inv_bt;
        qa.cs = reinterpret_cast<const double2*>(ws + L.off_cs); qa.gates = ws + L.off_U;
        qa.y = v.y; qa.bias = qn ? c.params : nullptr;
        qa.out = pr; qa.grad_x = gx; qa.partial = partial;
        qa.mrec = mrec; qa.ms = ms;
        // the members' launches of n >= 7 (one per n present); dense: BwdArgs::dense
        auto bwd_args = [&](int n, int dense) {
            return BwdArgs{two_runs(n, qs.dr.ld0, qs.dr.ld1), (long)v.nb, 0, 0, reinterpret_cast<const double2*>(ws + L.off_cs),
                           ws + L.off_U, 0, 0.0, 0.0, nullptr, nullptr, nullptr, v.y, qn ? c.params : nullptr, v.inv_bt, pr, gx,
                           partial, QHEA_PAULI_Z, 0, dense, nullptr};
        };
        profile_begin(st);
        for (int cl = 0; cl < kQsClasses; ++cl) {               // one launch per register class present
            if (plan.cls_count[cl] == 0) continue;
            qa.wk = QsWork{ws + L.off_list, plan.per, plan.cls_begin[cl]};
            const dim3 grid((unsigned)plan.cls_count[cl]);
            if (cl == 0) launch_bwd_qsweep_0(grid, st, qa);
            else launch_bwd_qsweep_1(grid, st, qa);
        }
        for (int n = kQsOwnLo; n <= kQsOwnHi; ++n) {            // n = 7..9: one launch per n present, member = blockIdx.y
            const int cnt = plan.own_count[n - kQsOwnLo];
            if (cnt == 0) continue;
            const long nw = qs_nwaves(n, v.nb);
            const BwdArgs ba = bwd_args(n, dense_bit(cnt * nw));
            const QubitArgs q{mrec, ms, QsWork{ws + L.off_list, plan.per, plan.own_begin[n - kQsOwnLo]}};
            const dim3 grid((unsigned)(nw / kWaves), (unsigned)cnt);
            switch (n) {
#define QHEA_CASE(NN) case NN: launch_bwd_qubit_##NN(grid, st, ba, q); break;
                QHEA_FOR_EACH_N(QHEA_CASE)
#undef QHEA_CASE
                default: return QHEA_EUNSUPPORTED;
            }
        }
        for (int n = kQsLdsLo; n <= kQsLdsHi; ++n) {            // n = 10..12: one launch per n present, one workgroup per
            const int cnt = plan.lds_count[n - kQsLdsLo];         // (sample, member)
            if (cnt == 0) continue;
            const QubitArgs q{mrec, ms, QsWork{ws + L.off_list, plan.per, plan.lds_begin[n - kQsLdsLo]}};
            const int rcl = launch_lds_bwd_qubit(n, dim3((unsigned)v.nb, (unsigned)cnt), st, bwd_args(n, 0), q);
            if (rcl != QHEA_OK) return rcl;
        }
        profile_end(st);
        if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
        const AdamStep as = adam_step(c, i, members[0].lr);
        hipLaunchKernelGGL((reduce_model_kernel<false, false, true, QubitRed>), dim3((unsigned)plan.red_count), dim3(kRedThreads), 0,
                           st, mi0.n, (int)mi0.sh.blk, padded_3n(mi0.n), 0L, (const double*)partial, (const double*)c.params,
                           (long)v.nb, (int)mi0.sh.E, enc, (const double*)gx, (const double*)pr, v.y, v.inv_bt, gm, 0, 0,
                           v.grad, as.adam, reinterpret_cast<const WorkspaceHeader*>(ws), (const double*)nullptr,
                           FusePrep{}, DpX{}, ms, MemberLr{mrec, as.bc1},
                           QubitRed{qs.dr, QsWork{ws + L.off_list, plan.per, plan.red_begin}});
        if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    }
    return QHEA_OK;
}

int qhea_model_qubit_sweep_train_steps(const qhea_model_desc* descs, int64_t n_models, const qhea_member_hparams* members,
                                       const double* ham_diag, int64_t n_steps, const int64_t* row_begin, const double* branch,
                                       const double* trunk, const double* y, double* params, const double* inv_batch_total,
                                       double* grad, int64_t grad_stride, double* exp_avg, double* exp_avg_sq,
                                       int64_t first_step, double beta1, double beta2, double eps, double weight_decay,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!descs || n_models < 1 || !members || n_steps < 1 || !row_begin || !inv_batch_total || !branch || !y || !grad ||
        first_step < 1)
        return QHEA_EINVAL;
    if (!member_records_ok(members, n_models, ham_diag)) return QHEA_EINVAL;
    QubitSet qs;
    const int rc0 = qubit_set(descs, n_models, qs);
    if (rc0 != QHEA_OK) return rc0;
    const TrainCall call{n_steps, row_begin, branch, trunk, y, params, inv_batch_total, grad, grad_stride, exp_avg, exp_avg_sq,
                         first_step, beta1, beta2, eps, weight_decay, workspace, workspace_bytes, stream};
    const int64_t bmax = call_max_batch(call, qs.pmax, descs[0]);
    if (bmax < 0) return QHEA_EINVAL;
    QubitPlan plan;
    qubit_plan(qs, bmax, plan);
    const size_t slice = qubit_slice_bytes(qs, bmax, plan.list_bytes);     // (every region grows with the batch)
    if (!workspace || slice == 0 || workspace_bytes < (size_t)n_models * slice) return QHEA_EWORKSPACE;
    return qubit_grid_steps(qs, plan, n_models, descs[0], members, ham_diag, slice, call);
}

int qhea_adam_step(int64_t n, double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t step,
                   double lr, double beta1, double beta2, double eps, double weight_decay, void* stream) {
    if (n < 0 || step < 1) return QHEA_EINVAL;
    if (n == 0) return QHEA_OK;
    if (!params || !grads || !exp_avg || !exp_avg_sq) return QHEA_EINVAL;
    const TrainCall opt = optimizer_call(params, exp_avg, exp_avg_sq, step, beta1, beta2, eps, weight_decay);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       (long)n, grads, adam_step(opt, 0, lr).adam);
    return hipGetLastError() == hipSuccess ? QHEA_OK : QHEA_ELAUNCH;
}

}  // extern "C"
