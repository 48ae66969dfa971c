// hea_lds.hpp -- the pass machinery of the workgroup-resident kernels (n = 10..12, state in LDS): the per-pass thread layout,
// the LDS index swizzle, the CNOT ring as an index map and the load / gate / store of a thread's 2^LG amplitudes.  Shared by
// hea_lds.hip (forward and backward sweeps), hea_noise_wide.hip and hea_noise_device_wide.hip (noisy trajectories); hea_lds.hip
// explains the scheme.  For the trajectory units (and hea_noise_grad_lds.hip, the sampled-trajectory gradient at n = 10..12) also
// the Pauli frame of a segment in this layout: ring_pull (Z through the ring), store_framed (the last pass's store with the frame
// applied), its mirror load_framed (a reverse layer's first gather) and the forward layer between them (noisy_layer); and the
// reverse layer on psi and lambda (inner, inner_x, bwd_layer), which hea_lds.hip's backward kernel shares with that unit.  The
// index and sign arithmetic of the two framed accesses (thread_part, group_slot, frame_neg) is __host__ __device__:
// tests/native/frame_mirror_check.cpp runs it on the host.
#pragma once
#include "hea_device.hpp"

namespace qhea {
namespace {

struct c2 { double x, y; };

constexpr int kFwdLG = 4;      // gate qubits per pass (see LCfg): forward kernel
#ifndef QHEA_LDS_BWD_LG
#define QHEA_LDS_BWD_LG 3
#endif
constexpr int kBwdLG = QHEA_LDS_BWD_LG;      // backward kernel

// LG = log2(amplitudes a thread holds per pass) = gate qubits per pass.  Forward kernel: 4 (256 threads at n = 12,
// two workgroups per CU).  Backward kernel: 3 (512 threads at n = 12, 248 VGPRs): psi + lambda fill the LDS, so one
// workgroup per CU, and the larger workgroup gives two waves per SIMD at the price of a fourth pass per layer --
// measured the two cancel almost exactly (forward + backward, LG = 3 / 4: n = 10 193 / 200 us, n = 11 410 / 415 us
// per 12 sub-layers, cfg 5 8.46 / 8.47 ms), LG = 3 kept.
template <int N, int LG>
struct LCfg {
    static_assert(N >= 10 && N <= 12, "workgroup-resident kernels: n = 10..12");
    static_assert(LG == 3 || LG == 4, "3 or 4 gate qubits per pass");
    static constexpr int M = 1 << LG;                 // amplitudes per thread and pass
    static constexpr int T = 1 << (N - LG);           // threads per sample
    static constexpr int NW = T / 64;                 // waves
    static constexpr int NP = (N + LG - 1) / LG;      // passes per gate layer
    static constexpr int DIM = 1 << N;
    static constexpr int KW = Cfg<N>::KW;             // padded 3n = row width of `partial` (reduce_kernel)
    static constexpr size_t STATE_BYTES = (size_t)16 << N;
    static constexpr size_t SCRATCH_BYTES = (size_t)NW * 64 * sizeof(double) + 16 * sizeof(double4);   // sums + gate table
};
template <int N, int P, int LG>
struct Pass {
    static constexpr int Q0 = LG * P;                                  // gate qubits [Q0, Q1)
    static constexpr int Q1 = (LG * P + LG < N) ? LG * P + LG : N;
    static constexpr int A = (LG * P + LG <= N) ? LG * P : N - LG;     // lowest of the LG index bits held per thread
};

// Which passes need a workgroup barrier between them.  thread_part maps the lane bits of a thread (t bits 0..5) and
// the pass's LG local bits onto index bits [0, 6 + LG) whenever A <= 6, and the wave number onto the bits above: the
// passes with A <= 6 (LG = 3: A = 0, 3, 6; LG = 4: A = 0, 4) all work on the SAME 2^(6+LG) amplitudes per wave.  Between
// two of them only the wave's own LDS accesses have to stay in order -- which the LDS pipe does for one wave's
// instructions -- so the waves of a workgroup drift apart there and one wave's LDS round trip overlaps another's
// arithmetic (with a barrier after every pass all waves load, compute and store in step: no overlap with one
// workgroup per CU).  Only the last pass (index bits above 6 + LG) exchanges amplitudes between waves.
template <int N, int LG, int PA, int PB>
constexpr bool wave_local_passes() { return Pass<N, PA, LG>::A <= 6 && Pass<N, PB, LG>::A <= 6; }
template <bool WAVE_LOCAL>
__device__ __forceinline__ void pass_sync() {
    if constexpr (WAVE_LOCAL) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // compiler ordering only: stores before ...
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");       // ... the next pass's loads
    } else {
        __syncthreads();
    }
}

// LDS index swizzle (an involution, linear over GF(2)): whatever the pass, the 16-byte accesses of 16 neighbouring
// lanes fall into 16 different bank quads.  LG = 4: bits 0..3 ^= bits 4..7.  LG = 3 (passes at bits 0, 3, 6, 9 or a
// ragged last one): bits 0..2 ^= bits 4..6 and bit 3 ^= bit 6.
template <int LG>
__host__ __device__ constexpr int phys(int k) {
    return LG == 4 ? (k ^ ((k >> 4) & 15)) : (k ^ ((k >> 4) & 7) ^ (((k >> 6) & 1) << 3));
}
// CNOT ring as a map of basis indices: |k> -> |ring(k)>, CNOT(control (i+1)%n, target i) for i = 0..n-1 in order
template <int N>
__host__ __device__ constexpr int ring_dst(int k) {
    for (int i = 0; i < N; ++i) k ^= ((k >> ((i + 1) % N)) & 1) << i;
    return k;
}
// z' with parity(ring(k) & z) = parity(k & z'): the transposed ring, last CNOT first
template <int N>
__host__ __device__ __forceinline__ int ring_pull(int z) {
#pragma unroll
    for (int i = N - 1; i >= 0; --i) z ^= ((z >> i) & 1) << ((i + 1) % N);
    return z;
}
// index bits of thread t for a pass with base bit A (the LG bits A..A+LG-1 are the per-thread local index j)
template <int A, int LG>
__host__ __device__ __forceinline__ int thread_part(int t) { return ((t >> A) << (A + LG)) | (t & ((1 << A) - 1)); }

// [[a,b],[-conj b, conj a]] on (p0,p1); u = (ar, ai, br, bi)
__device__ __forceinline__ void su2(c2& p0, c2& p1, const double4& u) {
    const c2 a0 = p0, a1 = p1;
    p0.x = u.x * a0.x - u.y * a0.y + u.z * a1.x - u.w * a1.y;
    p0.y = u.x * a0.y + u.y * a0.x + u.z * a1.y + u.w * a1.x;
    p1.x = u.x * a1.x + u.y * a1.y - u.z * a0.x - u.w * a0.y;
    p1.y = u.x * a1.y - u.y * a1.x - u.z * a0.y + u.w * a0.x;
}
__device__ __forceinline__ double4 dagger(double4 u) { return make_double4(u.x, -u.y, -u.z, -u.w); }
// RX as an SU(2) in the same form: a = c, b = -i s  ->  (c, 0, 0, -s)
__device__ __forceinline__ double4 rx_su2(double2 cs) { return make_double4(cs.x, 0.0, 0.0, -cs.y); }

// the 2^LG amplitudes of this thread for a pass with base bit A: local index j <-> index bits A..A+LG-1.
// `base` = phys(thread_part) (in place) or phys(ring(thread_part)) (through the ring); both maps are linear
// over GF(2), so amplitude j sits at base ^ group_slot(j).
template <int N, int A, bool RING, int LG>
__host__ __device__ constexpr int group_slot(int j) { return RING ? phys<LG>(ring_dst<N>(j << A)) : phys<LG>(j << A); }
template <int N, int A, bool RING, int LG>
__device__ __forceinline__ void load_group(const double2* s, int base, c2 (&v)[1 << LG]) {
    static_for<0, (1 << LG)>([&](auto jj) {
        constexpr int J = decltype(jj)::value;
        constexpr int CJ = group_slot<N, A, RING, LG>(J);
        const double2 a = s[base ^ CJ];
        v[J].x = a.x; v[J].y = a.y;
    });
}
template <int N, int A, bool RING, int LG>
__device__ __forceinline__ void store_group(double2* s, int base, const c2 (&v)[1 << LG]) {
    static_for<0, (1 << LG)>([&](auto jj) {
        constexpr int J = decltype(jj)::value;
        constexpr int CJ = group_slot<N, A, RING, LG>(J);
        s[base ^ CJ] = make_double2(v[J].x, v[J].y);
    });
}
// A Pauli frame behind a pass, psi'[k] = (-1)^parity(k & z) psi[k ^ x]: px = phys(x) moves the base (k -> k ^ x is linear like
// the ring and the swizzle), z signs the values (pulled back through the ring by the caller where RING); tp = the thread's index
// bits in this pass (thread_part).  frame_neg: the sign of local amplitude j, with sb = popcount(tp & z) and zl = frame_local(z).
template <int A, int LG>
__host__ __device__ __forceinline__ int frame_local(int z) { return (z >> A) & ((1 << LG) - 1); }
__host__ __device__ __forceinline__ bool frame_neg(int sb, int zl, int j) {
    return (sb + __builtin_popcount((unsigned)(j & zl))) & 1;
}
template <int A, int LG>
__device__ __forceinline__ void frame_signs(int z, int tp, c2 (&v)[1 << LG]) {
    if (z) {
        const int sb = __builtin_popcount((unsigned)(tp & z)), zl = frame_local<A, LG>(z);
        static_for<0, (1 << LG)>([&](auto jj) {
            constexpr int J = decltype(jj)::value;
            const bool neg = frame_neg(sb, zl, J);
            v[J].x = neg ? -v[J].x : v[J].x;
            v[J].y = neg ? -v[J].y : v[J].y;
        });
    }
}
// store_group behind the frame: a forward layer's last store (amplitude k goes to ring(k) ^ x with the sign of k & z)
template <int N, int A, bool RING, int LG>
__device__ __forceinline__ void store_framed(double2* s, int base, int px, int z, int tp, c2 (&v)[1 << LG]) {
    frame_signs<A, LG>(z, tp, v);
    store_group<N, A, RING, LG>(s, base ^ px, v);
}
// ... and its mirror, a reverse layer's first gather: amplitude k comes from ring(k) ^ x with the same sign, which undoes the
// store up to the sign (-1)^parity(x & z) that all amplitudes share
template <int N, int A, bool RING, int LG>
__device__ __forceinline__ void load_framed(const double2* s, int base, int px, int z, int tp, c2 (&v)[1 << LG]) {
    load_group<N, A, RING, LG>(s, base ^ px, v);
    frame_signs<A, LG>(z, tp, v);
}
template <int LBIT, int LG>
__device__ __forceinline__ void apply_group(c2 (&v)[1 << LG], const double4& u) {
    static_for<0, (1 << LG)>([&](auto jj) {
        constexpr int J = decltype(jj)::value;
        if constexpr (!(J & (1 << LBIT))) su2(v[J], v[J | (1 << LBIT)], u);
    });
}

template <int N, int LG>
struct Bases {                        // per-thread LDS index bases, computed once per kernel
    int plain[LCfg<N, LG>::NP];       // phys(thread_part<A_p>(t))
    int ring;                         // phys(ring(thread_part<A_last>(t)))
    __device__ __forceinline__ void init(int t) {
        static_for<0, LCfg<N, LG>::NP>([&](auto p) {
            constexpr int P = decltype(p)::value;
            plain[P] = phys<LG>(thread_part<Pass<N, P, LG>::A, LG>(t));
        });
        ring = phys<LG>(ring_dst<N>(thread_part<Pass<N, LCfg<N, LG>::NP - 1, LG>::A, LG>(t)));
    }
};

// One forward gate layer with a segment's frame behind it.  The last pass stores every amplitude where the ring (RING) and the X
// mask send it, with the Z mask's sign; `tpl` = the thread's index bits in that pass.  frame[0] = phys(x), frame[1] = z (pulled
// back through the ring where RING): written by thread 0 before the layer's last barrier pair and read between the two.
template <int N, bool RING, int LG, class G>
__device__ __forceinline__ void noisy_layer(double2* s, const Bases<N, LG>& bs, int tpl, const int* frame, G gate) {
    constexpr int NP = LCfg<N, LG>::NP;
    static_for<0, NP>([&](auto p) {
        constexpr int P = decltype(p)::value;
        using PS = Pass<N, P, LG>;
        c2 v[1 << LG];
        load_group<N, PS::A, false, LG>(s, bs.plain[P], v);
        static_for<PS::Q0, PS::Q1>([&](auto q) {
            constexpr int Q = decltype(q)::value;
            apply_group<Q - PS::A, LG>(v, gate(Q));
        });
        if constexpr (P < NP - 1) {
            store_group<N, PS::A, false, LG>(s, bs.plain[P], v);
            pass_sync<wave_local_passes<N, LG, P, P + 1>()>();
        } else {
            __syncthreads();                               // every thread holds its amplitudes: safe to permute
            const int px = __builtin_amdgcn_readfirstlane(frame[0]), z = __builtin_amdgcn_readfirstlane(frame[1]);
            store_framed<N, PS::A, RING, LG>(s, RING ? bs.ring : bs.plain[P], px, z, tpl, v);
            __syncthreads();
        }
    });
}

// Im<l|sigma|p> contributions of one pair (p0,p1),(l0,l1), accumulated as FMA chains: 4 fp64 instructions per product
// (written as sums of differences the compiler may not reassociate: mul, fma, mul, fma, add, add)
__device__ __forceinline__ void inner_x(const c2& p0, const c2& p1, const c2& l0, const c2& l1, double& X) {
    X = fma(l0.x, p1.y, X); X = fma(-l0.y, p1.x, X); X = fma(l1.x, p0.y, X); X = fma(-l1.y, p0.x, X);
}
__device__ __forceinline__ void inner(const c2& p0, const c2& p1, const c2& l0, const c2& l1, double& X, double& Y,
                                      double& Z) {
    inner_x(p0, p1, l0, l1, X);
    Y = fma(-l0.x, p1.x, Y); Y = fma(-l0.y, p1.y, Y); Y = fma(l1.x, p0.x, Y); Y = fma(l1.y, p0.y, Y);
    Z = fma(l0.x, p0.y, Z); Z = fma(-l0.y, p0.x, Z); Z = fma(-l1.x, p1.y, Z); Z = fma(l1.y, p1.x, Z);
}

// One reverse layer on psi and lambda: (ring^-1 via a gather in the first pass when RING), then per qubit the
// inner products Im<lam|sigma|psi> (XYZ: all three, else X only) followed by the adjoint gate on both states.
// gate(q, u) returns the ADJOINT coefficients.  acc: XYZ ? [3q..3q+2] : [q].
// FRAME: the layer undoes a segment whose forward store went through store_framed, so the first gather is load_framed with
// the same frame[0..1] and tpl (noisy_layer); the gather then leaves its own slots with or without a ring.  The caller has
// a barrier between thread 0's write of `frame` (and the previous layer's last store) and this call.
template <int N, int LG, bool RING, bool XYZ, bool FRAME = false, class G, int NA>
__device__ __forceinline__ void bwd_layer(double2* psi, double2* lam, const Bases<N, LG>& bs, G gate, double (&acc)[NA],
                                          const int* frame = nullptr, int tpl = 0) {
    constexpr int NP = LCfg<N, LG>::NP;
    static_rfor<0, NP>([&](auto p) {
        constexpr int P = decltype(p)::value;
        using PS = Pass<N, P, LG>;
        c2 v[1 << LG], l[1 << LG];
        if constexpr (FRAME && P == NP - 1) {
            const int px = __builtin_amdgcn_readfirstlane(frame[0]), z = __builtin_amdgcn_readfirstlane(frame[1]);
            load_framed<N, PS::A, RING, LG>(psi, RING ? bs.ring : bs.plain[P], px, z, tpl, v);
            load_framed<N, PS::A, RING, LG>(lam, RING ? bs.ring : bs.plain[P], px, z, tpl, l);
            __syncthreads();                               // all gathers done before anything is overwritten
        } else if constexpr (RING && P == NP - 1) {
            load_group<N, PS::A, true, LG>(psi, bs.ring, v);
            load_group<N, PS::A, true, LG>(lam, bs.ring, l);
            __syncthreads();                               // all gathers done before anything is overwritten
        } else {
            load_group<N, PS::A, false, LG>(psi, bs.plain[P], v);
            load_group<N, PS::A, false, LG>(lam, bs.plain[P], l);
        }
        static_for<PS::Q0, PS::Q1>([&](auto q) {
            constexpr int Q = decltype(q)::value;
            constexpr int LBIT = Q - PS::A;
            double4 u;
            if (gate(Q, u)) {
                static_for<0, (1 << LG)>([&](auto jj) {
                    constexpr int J = decltype(jj)::value;
                    if constexpr (!(J & (1 << LBIT))) {
                        constexpr int J1 = J | (1 << LBIT);
                        if constexpr (XYZ) inner(v[J], v[J1], l[J], l[J1], acc[3 * Q], acc[3 * Q + 1], acc[3 * Q + 2]);
                        else inner_x(v[J], v[J1], l[J], l[J1], acc[Q]);
                        su2(v[J], v[J1], u);
                        su2(l[J], l[J1], u);
                    }
                });
            }
        });
        store_group<N, PS::A, false, LG>(psi, bs.plain[P], v);
        store_group<N, PS::A, false, LG>(lam, bs.plain[P], l);
        // the next pass: P - 1, or the last pass of the following (earlier) layer
        pass_sync<(P > 0) && wave_local_passes<N, LG, P, (P > 0 ? P - 1 : 0)>()>();
    });
}

// sum of one double per thread over the workgroup -- the wave by the xor butterfly (offsets 32 .. 1), then the NW waves in wave
// order through red[NW] -- in every thread; the caller has a barrier before red is written again
template <int NW>
__device__ __forceinline__ double wide_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if constexpr (NW == 1) return v;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double tot = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) tot += red[w];
    return tot;
}

}  // namespace
}  // namespace qhea
