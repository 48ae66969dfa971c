// hea_noise_jump_lds.hpp -- the quantum-jump walk in the LDS layout (n = 10..12): what hea_noise_device_wide.hip (the forward,
// qhea_model_forward_noisy_device_wide) and hea_noise_device_grad_lds.hip (its gradient, qhea_model_*_noisy_device_lds) share.
// The scratch in front of the state, the stored-bit mask of a ring site, a site's workgroup sum, the relaxation of a site as a
// diagonal step on the 16 amplitudes a thread holds (relax_site), the segment's draws (segment_draws), the gate layer with its
// sites (jump_layer) and the layer without sites (plain_layer).  hea_noise_device_wide.hip explains the scheme.
//
// jump_layer reports what it decided to a recorder: rec.site<IDX>(xq, fired) behind site IDX of the segment (0..n-1 the layer's
// own sites, n + 2 j the TGT and n + 2 j + 1 the CTL site of slot j) with the frame's X bit on the site's wire when the site was
// reached and whether the jump fired, and rec.tail(px, z, rescaled) in front of the last store with the frame that store applies.
// The forward kernel passes NoRecord, whose calls are empty; the gradient kernel keeps the words for its reverse walk.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#include "hea_lds.hpp"
#include "hea_noise_jump.hpp"

namespace qhea {
namespace {

constexpr int kLG = 4;                      // gate qubits per pass, as noisy_wide_lds_kernel
// In FRONT of the state: at n = 12 the state alone fills the 64 KiB an LDS instruction's immediate offset reaches, and behind it
// every scratch word would need its address in a register (36 draws: scalar registers that spill inside the sub-layer loop)
struct JumpScratch {
    double red[2][4];                       // a site's per-wave sums, two alternating sets
    double rsum[2][4];                      // the read-out's per-wave sums (numerator / cdf, total)
    int lo[4], hi[4];                       // per-wave first hit / last positive index
    unsigned code[3 * kWideWires], w3[3 * kWideWires];   // the segment's draws
    int m01, m10;                           // shot mode: the bits that flip when read as 0 / as 1
    double u;
};
constexpr size_t kScratchBytes = 512;       // a multiple of the LDS bank period: the swizzle of phys<4> sees the same banks
static_assert(sizeof(JumpScratch) <= kScratchBytes, "the state starts behind the scratch");

// The stored-bit mask of the wire of a ring site behind slot J, the state in pre-ring labels (CNOT(c = J + 1 -> t = J) applied
// for slots 0..J): TGT is wire J, CTL wire (J + 1) mod N
template <int N, int J, bool TGT>
constexpr int ring_site_mask() {
    if (TGT) return J < N - 1 ? (1 << J) | (1 << (J + 1)) : (1 << (N - 1)) | 3;
    return J < N - 1 ? 1 << (J + 1) : 3;
}

// What every thread carries along a trajectory; all values are the same in every thread of the workgroup
struct JumpState {
    double n2;                              // squared norm of the stored state
    int x, z;                               // the frame, in the labels of the circuit point reached
    int par;                                // which slot set the next reduction writes
};

struct NoRecord {
    template <int IDX>
    __device__ __forceinline__ void site(int, int) {}
    __device__ __forceinline__ void tail(int, int, bool) {}
};

// v summed over the workgroup: the butterfly over the wave, offsets 32 .. 1, then the waves in order
template <int NW>
__device__ __forceinline__ double site_sum(double v, JumpScratch* sc, int& par) {
    v = group_sum<6>(v);
    if constexpr (NW == 1) {
        return v;
    } else {
        if ((threadIdx.x & 63) == 0) sc->red[par][threadIdx.x >> 6] = v;
        __syncthreads();
        double tot = sc->red[par][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) tot += sc->red[par][w];
        par ^= 1;
        return tot;
    }
}

// Dephasing and damping of one site on wire W, whose |1> is the parity of the stored bits MASK; the thread holds the amplitudes
// tp | J << A.  c, w3: the site's code and jump word; gs = (gamma, sqrt(1 - gamma)).
template <int N, int A, int W, int MASK>
__device__ __forceinline__ void relax_site(c2 (&v)[1 << kLG], JumpState& js, int tp, unsigned c, unsigned w3, double2 gs,
                                           JumpScratch* sc) {
    constexpr int M16 = 1 << kLG, ML = (MASK >> A) & (M16 - 1);
    const double g = gs.x, s = gs.y;
    js.z ^= (int)((c >> 4) & 1u) << W;
    if (g > 0.0) {                                                       // workgroup-uniform: a table entry
        const int pol = (__popc((unsigned)(tp & MASK)) + ((js.x >> W) & 1)) & 1;
        double m = 0.0;
        static_for<0, M16>([&](auto jj) {
            constexpr int J = decltype(jj)::value;
            const bool one = pol != (__builtin_popcount(J & ML) & 1);
            m += one ? v[J].x * v[J].x + v[J].y * v[J].y : 0.0;
        });
        m = site_sum<LCfg<N, kLG>::NW>(m, sc, js.par);
        const bool fire = uniform(jump_u(w3) * js.n2 < g * m);           // the same in every thread
        if (fire) {
            static_for<0, M16>([&](auto jj) {
                constexpr int J = decltype(jj)::value;
                const bool one = pol != (__builtin_popcount(J & ML) & 1);
                v[J].x = one ? v[J].x : 0.0; v[J].y = one ? v[J].y : 0.0;
            });
            js.n2 = m;
            js.x ^= 1 << W;
        } else {
            static_for<0, M16>([&](auto jj) {
                constexpr int J = decltype(jj)::value;
                const bool one = pol != (__builtin_popcount(J & ML) & 1);
                const double f = one ? s : 1.0;
                v[J].x *= f; v[J].y *= f;
            });
            js.n2 -= g * m;
        }
    }
}

// Wave 0's lanes draw the segment's calls call0 .. call0 + cnt - 1 (template entries tbase ..; RING: the calls from `ring0` on
// alternate pair Pauli / none) into the scratch; the barrier behind it opens the layer.  a.thr1 == 0: an ideal setting.
__device__ __forceinline__ void segment_draws(const NoiseArgs& a, const WideDevTable* __restrict__ tab, JumpScratch* sc,
                                              unsigned call0, int tbase, int cnt, int ring0, unsigned traj, unsigned long long row) {
    const int c = threadIdx.x;
    if (c < cnt) {
        unsigned code = 0, w3 = 0;
        if (a.thr1 != 0) {
            // the key behind a fence: without it the ten round keys of each word are loop invariants that the compiler keeps in
            // scalar registers across the circuit loop, where they spill; behind it they are nine scalar adds per call
            unsigned k0 = a.key0, k1 = a.key1;
            asm volatile("" : "+s"(k0), "+s"(k1));
            const uint4 w = philox(make_uint4(call0 + (unsigned)c, traj, (unsigned)row, (unsigned)(row >> 32)), k0, k1);
            draw_code(tab, tbase + c, w, (c >= ring0 && !((c - ring0) & 1)) ? 15u : 3u, code, w3);
        }
        sc->code[c] = code; sc->w3[c] = w3;
    }
    __syncthreads();
}

// One gate layer with its sites.  SITE: kEnc (a block's encoding layer, no ring) or kRot (a sub-layer: its ring's 2 n sites sit
// in the last pass and the ring is that pass's scatter).  The frame, the power-of-two rescale and the ring go into the last
// pass's store.
template <int N, int SITE, class G, class Rec>
__device__ __forceinline__ void jump_layer(double2* s, const Bases<N, kLG>& bs, int t, JumpScratch* sc,
                                           const WideDevTable* __restrict__ tab, JumpState& js, G gate, Rec& rec) {
    constexpr int LG = kLG, NP = LCfg<N, LG>::NP;
    constexpr bool RING = SITE == kRot;
    static_for<0, NP>([&](auto p) {
        constexpr int P = decltype(p)::value;
        using PS = Pass<N, P, LG>;
        const int tp = thread_part<PS::A, LG>(t);
        c2 v[1 << LG];
        load_group<N, PS::A, false, LG>(s, bs.plain[P], v);
        static_for<PS::Q0, PS::Q1>([&](auto q) {
            constexpr int Q = decltype(q)::value;
            apply_group<Q - PS::A, LG>(v, gate(Q));
            const unsigned c = (unsigned)uniform((int)sc->code[Q]), w3 = (unsigned)uniform((int)sc->w3[Q]);
            js.x ^= pauli_x(c & 3u, Q); js.z ^= pauli_z(c & 3u, Q);
            const int xb = js.x;
            relax_site<N, PS::A, Q, (1 << Q)>(v, js, tp, c, w3, site_pair(tab, SITE, Q), sc);
            rec.template site<Q>((xb >> Q) & 1, ((xb ^ js.x) >> Q) & 1);
        });
        if constexpr (P < NP - 1) {
            store_group<N, PS::A, false, LG>(s, bs.plain[P], v);
            pass_sync<wave_local_passes<N, LG, P, P + 1>()>();
        } else {
            if constexpr (RING) {
                static_for<0, N>([&](auto jj) {                          // slot j: CNOT(c -> t), pair Pauli, TGT of t, CTL of c
                    constexpr int J = decltype(jj)::value, CQ = (J + 1) % N, TQ = J;
                    js.x ^= ((js.x >> CQ) & 1) << TQ;
                    js.z ^= ((js.z >> TQ) & 1) << CQ;
                    const unsigned c0 = (unsigned)uniform((int)sc->code[N + 2 * J]), c1 = (unsigned)uniform((int)sc->code[N + 2 * J + 1]);
                    const unsigned u0 = (unsigned)uniform((int)sc->w3[N + 2 * J]), u1 = (unsigned)uniform((int)sc->w3[N + 2 * J + 1]);
                    const unsigned pp = c0 & 15u;
                    js.x ^= pauli_x(pp >> 2, CQ) | pauli_x(pp & 3u, TQ);
                    js.z ^= pauli_z(pp >> 2, CQ) | pauli_z(pp & 3u, TQ);
                    const int xt = js.x;
                    relax_site<N, PS::A, TQ, ring_site_mask<N, J, true>()>(v, js, tp, c0, u0, site_pair(tab, kTgt, TQ), sc);
                    rec.template site<N + 2 * J>((xt >> TQ) & 1, ((xt ^ js.x) >> TQ) & 1);
                    const int xc = js.x;
                    relax_site<N, PS::A, CQ, ring_site_mask<N, J, false>()>(v, js, tp, c1, u1, site_pair(tab, kCtl, CQ), sc);
                    rec.template site<N + 2 * J + 1>((xc >> CQ) & 1, ((xc ^ js.x) >> CQ) & 1);
                });
            }
            const bool rescale = js.n2 < 0x1p-200;
            if (rescale) {                                               // exact, so invisible in the result
                static_for<0, (1 << LG)>([&](auto jj) {
                    constexpr int J = decltype(jj)::value;
                    v[J].x *= 0x1p100; v[J].y *= 0x1p100;
                });
                js.n2 *= 0x1p200;
            }
            __syncthreads();                               // every thread holds its amplitudes: safe to permute
            const int px = phys<LG>(js.x), z = RING ? ring_pull<N>(js.z) : js.z;
            rec.tail(px, z, rescale);
            store_framed<N, PS::A, RING, LG>(s, RING ? bs.ring : bs.plain[P], px, z, tp, v);
            js.x = 0; js.z = 0;
            __syncthreads();
        }
    });
}

// ---- what a walk back needs of a walked segment (hea_noise_device_grad_lds.hip).  The arithmetic is __host__ __device__:
// tests/native/jump_site_check.cpp runs it on the host.

// relax_site's predicate as a function: amplitude tp | j << A has the wire whose |1> is the parity of the stored bits MASK
// reading |1> under the frame's X bit xq
template <int A, int MASK>
__host__ __device__ __forceinline__ bool wire_reads_one(int tp, int xq, int j) {
    constexpr int ML = (MASK >> A) & ((1 << kLG) - 1);
    return ((__builtin_popcount((unsigned)(tp & MASK)) + xq + __builtin_popcount((unsigned)(j & ML))) & 1) != 0;
}

// A segment's record: bit IDX of `fired` / `pol`: site IDX fired / the frame's X bit on its wire when it was reached (IDX < n
// the layer's own site of wire IDX, n + 2 j the TGT and n + 2 j + 1 the CTL site of slot j); px, z: what the segment's last
// store was framed with; rescaled: the 2^100 rescale fired.  Six 32-bit words of the eight a segment has in the workspace.
struct SegWords {
    unsigned long long fired, pol;
    int px, z;
    bool rescaled;
};
constexpr int kSegWords = 8;
__host__ __device__ __forceinline__ void pack_words(const SegWords& v, unsigned (&w)[6]) {
    w[0] = (unsigned)v.fired; w[1] = (unsigned)(v.fired >> 32) | (v.rescaled ? 1u << 31 : 0u);
    w[2] = (unsigned)v.pol; w[3] = (unsigned)(v.pol >> 32);
    w[4] = (unsigned)v.px; w[5] = (unsigned)v.z;
}
__host__ __device__ __forceinline__ SegWords unpack_words(const unsigned (&w)[6]) {
    SegWords v;
    v.fired = (unsigned long long)w[0] | ((unsigned long long)(w[1] & 0x7FFFFFFFu) << 32);
    v.pol = (unsigned long long)w[2] | ((unsigned long long)w[3] << 32);
    v.px = (int)w[4]; v.z = (int)w[5];
    v.rescaled = (w[1] >> 31) != 0u;
    return v;
}

// One gate layer without sites: the X / Y basis change
template <int N, class G>
__device__ __forceinline__ void plain_layer(double2* s, const Bases<N, kLG>& bs, G gate) {
    constexpr int LG = kLG, NP = LCfg<N, LG>::NP;
    static_for<0, NP>([&](auto p) {
        constexpr int P = decltype(p)::value;
        using PS = Pass<N, P, LG>;
        c2 v[1 << LG];
        load_group<N, PS::A, false, LG>(s, bs.plain[P], v);
        static_for<PS::Q0, PS::Q1>([&](auto q) { apply_group<decltype(q)::value - PS::A, LG>(v, gate(decltype(q)::value)); });
        store_group<N, PS::A, false, LG>(s, bs.plain[P], v);
        __syncthreads();
    });
}

}  // namespace
}  // namespace qhea
