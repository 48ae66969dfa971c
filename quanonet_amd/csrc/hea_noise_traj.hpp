// hea_noise_traj.hpp -- what the noisy entry points share.  All units (hea_noise.hip, hea_noise_wide.hip, hea_noise_device.hip,
// hea_noise_device_wide.hip and the density-matrix ones): the checks of a qhea_noise and the argument checks that open every call
// (noisy_call_check).  The four trajectory units (uniform noise at n = 2..6, one amplitude per lane, and at n = 7..12, registers
// or LDS; device noise at n = 2..9 in both register layouts and at n = 10..12 in LDS): the argument record, the Philox stream and its error codes, the Pauli frame bits and the frame's
// application in either layout (apply_frame, frame_regs), the work item, wave_scan, u and the value of a shot, the workspace
// layout, and the head and tail of the entry point around a unit's kernels (traj_open, traj_finish); the uniform model's segment
// frames (enc_frame, sub_frame), readout_weight and the launch of the readout mix, which hea_noise_wide.hip shares with the
// sampled-trajectory gradient unit (hea_noise_grad.hip).  What only the two
// device-noise units share (their table, its prep kernel's body, the site helpers, the entry point's body) is
// hea_noise_jump.hpp's; the frame in the LDS layout (ring_pull, store_framed) is hea_lds.hpp's.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "hea_model.hpp"
#include "hea_train.hpp"

namespace qhea {

constexpr int kTile = 64;                   // trajectories per work item (fixes the summation order: part of the contract)

struct NoiseArgs {
    const double4* gates;                   // prep table, entry 0 = padding entry -n
    const double2* cs;                      // [B, E]
    const double* diag;                     // ham_diag or NULL
    const double* bias;                     // model bias or NULL
    double off, co, q;                      // H = off + co sum P_i; readout flip probability
    unsigned long long thr1, thr2, thrq;    // an event happens iff word < thr (thr = p 2^32)
    long B, row0, T;                        // rows, global index of row 0, values (trajectories or shots) per row
    int tiles, E, pauli, shots;             // tiles per row; shots != 0: shot mode
    int nb[2], ld[2];
    unsigned key0, key1;
    unsigned L;                             // noise locations of the circuit
    double2* partial;                       // [B * tiles] (sum, sum of squares)
};

// Philox4x32-10 (Salmon et al., SC'11; the Random123 reference constants)
__device__ __forceinline__ uint4 philox(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c.z;
        c = make_uint4((unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0);
    }
    return c;
}

// error codes of this lane's call (l0 / 2 + k) for the segment [l0, l0 + cnt) whose first n1 locations are one-qubit channels:
// byte h = code of location 2c + h (0: no error; 1..3 one-qubit Pauli X, Y, Z; 1..15 two-qubit pair (code >> 2, code & 3))
__device__ __forceinline__ unsigned segment_codes(const NoiseArgs& a, unsigned l0, unsigned cnt, unsigned n1, unsigned traj,
                                                  unsigned long long row, int k) {
    if ((a.thr1 | a.thr2) == 0) return 0;
    const unsigned c = (l0 >> 1) + (unsigned)k;
    const uint4 w = philox(make_uint4(c, traj, (unsigned)row, (unsigned)(row >> 32)), a.key0, a.key1);
    unsigned out = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const unsigned l = 2 * c + h;
        if (l >= l0 && l < l0 + cnt) {
            const bool two = l - l0 >= n1;
            const unsigned w0 = h ? w.z : w.x, w1 = h ? w.w : w.y;
            if ((unsigned long long)w0 < (two ? a.thr2 : a.thr1))
                out |= (1u + (unsigned)(((unsigned long long)w1 * (two ? 15u : 3u)) >> 32)) << (8 * h);
        }
    }
    return out;
}

__device__ __forceinline__ unsigned code_at(unsigned codes, unsigned l0, unsigned l, int base) {
    return (__shfl(codes, base + (int)((l >> 1) - (l0 >> 1))) >> (8 * (l & 1))) & 255u;
}

// Pauli p (0 I, 1 X, 2 Y, 3 Z) on wire w as (X mask, Z mask) bits, up to phase
__device__ __forceinline__ int pauli_x(unsigned p, int w) { return (p == 1u || p == 2u) ? 1 << w : 0; }
__device__ __forceinline__ int pauli_z(unsigned p, int w) { return p >= 2u ? 1 << w : 0; }

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// u in [0, 1) of shot mode's cdf search: 53 bits from two words
__device__ __forceinline__ double unit_double(unsigned w0, unsigned w1) {
    return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) * 0x1p-53;
}

template <int N>
__device__ __forceinline__ double shot_value(const double* __restrict__ diag, double off, double co, int out) {
#pragma clang fp contract(off)              // a product and a sum, each rounded: a shot's value is the same number on any host
    return diag ? diag[out] : off + co * (double)(N - 2 * (int)__popc((unsigned)out));
}

// A work item of the wave kernels and the LDS kernel: row r of the call (global row `row`, its encoding table csr) and the
// tcount <= kTile trajectories from t0 on
struct WorkItem {
    long r, t0;
    int tcount;
    unsigned long long row;
    const double2* csr;
};
__device__ __forceinline__ WorkItem work_item(const NoiseArgs& a, long item) {
    const long r = item / a.tiles, t0 = (item - r * a.tiles) * (long)kTile;
    return {r, t0, (int)(a.T - t0 < kTile ? a.T - t0 : kTile), (unsigned long long)(a.row0 + r), a.cs + r * a.E};
}

// one amplitude per lane (n = 2..6), basis state k of a slot on lane base + k: psi <- X^x Z^z psi (up to a global phase),
// psi'[k] = (-1)^popcount((k ^ x) & z) psi[k ^ x]
__device__ __forceinline__ void apply_frame(double& re, double& im, int x, int z, int k, int base) {
    if (__any(x | z)) {
        const int src = k ^ x;
        const double pr = __shfl(re, base + src), pi = __shfl(im, base + src);
        const bool neg = __popc(src & z) & 1;
        re = neg ? -pr : pr;
        im = neg ? -pi : pi;
    }
}

// inclusive sum over the lanes 0 .. lane of a wave (Hillis-Steele, distances 1, 2, .. 32: a fixed order)
__device__ __forceinline__ double wave_scan(double c, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double t = __shfl_up(c, d);
        if (lane >= d) c += t;
    }
    return c;
}

// Cfg<N>'s register layout (n = 7..9), k = lane | r << 6: psi'[k] = (-1)^parity(k & z) psi[k ^ x]; x, z wave-uniform
template <int N>
__device__ __forceinline__ void frame_regs(double (&re)[Cfg<N>::R], double (&im)[Cfg<N>::R], int x, int z, int lane) {
    using C = Cfg<N>;
    if ((x | z) == 0) return;
    if (x & 63) {
        const int src = (lane ^ (x & 63)) << 2;
#pragma unroll
        for (int r = 0; r < C::R; ++r) { re[r] = lane_gather(re[r], src); im[r] = lane_gather(im[r], src); }
    }
    static_for<0, C::RB>([&](auto b) {
        constexpr int J = 1 << decltype(b)::value;
        if ((x >> 6) & J) {
#pragma unroll
            for (int r = 0; r < C::R; ++r) {
                if (r & J) continue;
                double t = re[r]; re[r] = re[r | J]; re[r | J] = t;
                t = im[r]; im[r] = im[r | J]; im[r | J] = t;
            }
        }
    });
    if (z) {
        const int lp = __popc((unsigned)(lane & z & 63));
#pragma unroll
        for (int r = 0; r < C::R; ++r) {
            const bool neg = (lp + __popc((unsigned)(r & (z >> 6)))) & 1;
            re[r] = neg ? -re[r] : re[r];
            im[r] = neg ? -im[r] : im[r];
        }
    }
}

// The frames of the uniform model's segments (hea_noise_wide.hip's forward walk, hea_noise_grad.hip's walk both ways).
// (X mask, Z mask) of the errors behind a block's n encoding RX gates; codes: segment_codes of the wave's lanes
template <int N>
__device__ __forceinline__ void enc_frame(unsigned codes, unsigned loc, int& x, int& z) {
    x = 0; z = 0;
    if (!__any(codes != 0u)) return;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const unsigned p = code_at(codes, loc, loc + q, 0);
        x |= pauli_x(p, q); z |= pauli_z(p, q);
    }
    x = uniform(x); z = uniform(z);
}
// ... of a sub-layer, as one frame behind its ring: the rotations' errors, then per CNOT(c -> t) the conjugation and its own
template <int N>
__device__ __forceinline__ void sub_frame(unsigned codes, unsigned loc, int& x, int& z) {
    x = 0; z = 0;
    if (!__any(codes != 0u)) return;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const unsigned p = code_at(codes, loc, loc + q, 0);
        x |= pauli_x(p, q); z |= pauli_z(p, q);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int c = (j + 1) % N, t = j;
        x ^= ((x >> c) & 1) << t;
        z ^= ((z >> t) & 1) << c;
        const unsigned p = code_at(codes, loc, loc + N + j, 0);
        x ^= pauli_x(p >> 2, c) | pauli_x(p & 3u, t);
        z ^= pauli_z(p >> 2, c) | pauli_z(p & 3u, t);
    }
    x = uniform(x); z = uniform(z);
}

// expectation mode's weight of basis state k (hd: the readout-confused ham_diag, or NULL)
template <int N>
__device__ __forceinline__ double readout_weight(const NoiseArgs& a, const double* __restrict__ hd, int k) {
    return hd ? hd[k] : a.co * (1.0 - 2.0 * a.q) * (double)(N - 2 * (int)__popc((unsigned)k));
}

// readout_mix_kernel (hea_noise_wide.hip) on `st`: ham_diag under the readout confusion, built bit by bit in mix[2 * 2^n];
// *hd = where the table ends up (the half (n - 1) & 1)
int launch_readout_mix(const double* diag, double q, int n, double* mix, hipStream_t st, const double** hd);

// an event happens iff its 32-bit word is < threshold(p) (p 2^32, floored)
inline unsigned long long threshold(double p) { return (unsigned long long)(p * 4294967296.0); }

inline bool rates_ok(const qhea_noise* nz) {
    if (!nz) return false;
    for (double p : {nz->p1, nz->p2, nz->readout})
        if (!(p >= 0.0 && p <= 1.0)) return false;
    return true;
}

// values per row (T trajectories or S shots), or QHEA_EINVAL
inline int64_t noise_values(const qhea_noise* nz) {
    if (!rates_ok(nz) || nz->shots < 0) return QHEA_EINVAL;
    const int64_t T = nz->shots > 0 ? nz->shots : nz->trajectories;
    if (T < 1 || T > (int64_t)0xFFFFFFFF) return QHEA_EINVAL;          // trajectory index is one 32-bit counter word
    return T;
}

// log10 of the factor the gradient's inverse walk amplifies the traceless part of rho by; +inf for a singular channel
inline double log10_amplification(const ModelInfo& mi, const qhea_noise* nz) {
    const double k1 = 1.0 - 4.0 * nz->p1 / 3.0, k2 = 1.0 - 16.0 * nz->p2 / 15.0;
    if (!(k1 > 0.0) || !(k2 > 0.0)) return INFINITY;
    const double L1 = (double)mi.sh.E + (double)mi.n * mi.sh.blk, L2 = (double)mi.n * mi.sh.blk;
    return -(L1 * log10(k1) + L2 * log10(k2));
}
constexpr double kMaxLog10Amplification = 12.0;

// What differs between the noisy calls' checks: the qubit counts the call's kernels exist for, whether the noise setting
// carries a value count (trajectory calls) or rates only, and whether the call walks the channels back (gradient calls)
struct NoisyKind { int nmin, nmax; bool trajectories, inverse_walk; };
// What a call knows once it has passed them
struct NoisyCall {
    ModelInfo mi;
    int64_t T = 0;                          // values per row (trajectory calls)
    bool empty = false;                     // QHEA_OK and nothing to do
    hipStream_t st = nullptr;
    char* ws = nullptr;
};
// Everything a noisy call is refused for before it sizes its workspace, in the order the ABI reports it: the descriptor, the
// noise setting, the qubit range (QHEA_EUNSUPPORTED), the read-out, the conditioning (QHEA_EUNSUPPORTED), then count < 0 or
// row0 < 0, count == 0 (QHEA_OK, c.empty) and the pointers the call cannot do without (`required`, and a QuanONet's trunk).
// count: the rows of the call, or the steps of a schedule; row0: 0 where the call has none.
inline int noisy_call_check(const NoisyKind& k, const qhea_model_desc* desc, const double* ham_diag, const qhea_noise* noise,
                            int64_t row0, int64_t count, const double* trunk, std::initializer_list<const void*> required,
                            void* workspace, void* stream, NoisyCall& c) {
    const int rc = model_info(desc, c.mi);
    if (rc != QHEA_OK) return rc;
    if (k.trajectories) c.T = noise_values(noise);
    if (k.trajectories ? c.T < 1 : !rates_ok(noise)) return QHEA_EINVAL;
    if (c.mi.n < k.nmin || c.mi.n > k.nmax) return QHEA_EUNSUPPORTED;
    if (!pauli_ok(desc->ham_pauli, ham_diag)) return QHEA_EINVAL;
    if (k.inverse_walk && !(log10_amplification(c.mi, noise) <= kMaxLog10Amplification)) return QHEA_EUNSUPPORTED;
    if (count < 0 || row0 < 0) return QHEA_EINVAL;
    c.empty = count == 0;
    if (c.empty) return QHEA_OK;
    for (const void* p : required)
        if (!p) return QHEA_EINVAL;
    if (desc->model == QHEA_MODEL_QUANONET && !trunk) return QHEA_EINVAL;
    c.st = static_cast<hipStream_t>(stream);
    c.ws = static_cast<char*>(workspace);
    return QHEA_OK;
}

// everything of NoiseArgs that the descriptor and the noise setting fix; the caller adds the workspace pointers
inline NoiseArgs noise_args(const qhea_model_desc* desc, const ModelInfo& mi, const qhea_noise* noise, const double* params,
                            const double* ham_diag, int64_t row0, int64_t batch, int64_t T) {
    NoiseArgs a{};
    a.diag = ham_diag;
    a.bias = mi.has_bias ? params + mi.off_bias : nullptr;
    a.off = desc->ham_offset; a.co = desc->ham_coeff; a.q = noise->readout;
    a.thr1 = threshold(noise->p1); a.thr2 = threshold(noise->p2); a.thrq = threshold(noise->readout);
    a.B = batch; a.row0 = row0; a.T = T; a.tiles = (int)((T + kTile - 1) / kTile); a.E = (int)mi.sh.E; a.pauli = desc->ham_pauli;
    a.shots = noise->shots > 0 ? 1 : 0;
    unsigned locs = 0;
    for (int g = 0; g < 2; ++g) {
        a.nb[g] = mi.nb[g]; a.ld[g] = mi.ld[g];
        locs += (unsigned)mi.nb[g] * (unsigned)(mi.n + 2 * mi.n * mi.ld[g]);
    }
    a.L = locs;
    a.key0 = (unsigned)noise->seed; a.key1 = (unsigned)(noise->seed >> 32);
    return a;
}

// noisy_finish_kernel (hea_noise.hip) on `st`: row r's tiles added in tile order, mean (+ bias) and standard error
int launch_noisy_finish(const double2* partial, int tiles, int64_t B, int64_t T, const double* bias, double* pred, double* se,
                        hipStream_t st);

// A trajectory unit: the qubit counts of its kernels, whether it keeps ham_diag under the readout confusion in a region of its
// own (`wide`: 2 x 2^n doubles), and the bytes of a last region of its own (0: none)
struct TrajUnit {
    int nmin, nmax;
    bool wide;
    size_t extra;
};

struct TrajLayout { size_t off_gates, off_cs, off_part, off_mix /* wide units */, off_extra, total; int tiles; };
inline TrajLayout traj_layout(const TrajUnit& u, const ModelInfo& mi, int64_t B, int64_t T) {
    TrajLayout L{};
    L.tiles = (int)((T + kTile - 1) / kTile);
    const TableLayout t = table_layout(mi, B);
    L.off_gates = t.off_gates; L.off_cs = t.off_cs;
    size_t p = t.end;
    L.off_part = p; p = align256(p + (size_t)B * L.tiles * sizeof(double2));
    if (u.wide) { L.off_mix = p; p = align256(p + ((size_t)2 << mi.n) * sizeof(double)); }
    if (u.extra) { L.off_extra = p; p = align256(p + u.extra); }
    L.total = p;
    return L;
}

// qhea_model_noisy_workspace_bytes answers for every qubit count, the wide units' calls for their own counts only
inline size_t traj_workspace_bytes(const TrajUnit& u, const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise) {
    ModelInfo mi;
    const int64_t T = noise_values(noise);
    if (T < 1 || batch < 0 || model_info(desc, mi) != QHEA_OK || (u.wide && (mi.n < u.nmin || mi.n > u.nmax))) return 0;
    return traj_layout(u, mi, batch, T).total;
}

// What a trajectory call holds once traj_open has passed it: the regions of its workspace and its kernels' arguments
struct TrajCall {
    NoisyCall c;
    TrajLayout L;
    NoiseArgs a;
    double* mix = nullptr;                  // wide units
    char* extra = nullptr;                  // units with a region of their own
};

// The head of the three trajectory entry points: checks, layout, prep.  QHEA_OK with t.c.empty set: nothing to do.
inline int traj_open(const TrajUnit& u, const qhea_model_desc* desc, int64_t row0, int64_t batch, const double* branch,
                     const double* trunk, const double* params, const double* ham_diag, const qhea_noise* noise, double* pred,
                     void* workspace, size_t workspace_bytes, void* stream, TrajCall& t) {
    NoisyCall& c = t.c;
    int rc = noisy_call_check({u.nmin, u.nmax, true, false}, desc, ham_diag, noise, row0, batch, trunk, {branch, params, pred},
                              workspace, stream, c);
    if (rc != QHEA_OK || c.empty) return rc;
    const TrajLayout& L = t.L = traj_layout(u, c.mi, batch, c.T);
    if (!workspace || workspace_bytes < L.total) return QHEA_EWORKSPACE;
    if (u.wide && (int64_t)batch * L.tiles > (int64_t)INT_MAX) return QHEA_EINVAL;      // one workgroup per (row, tile)
    double4* gates = reinterpret_cast<double4*>(c.ws + L.off_gates);
    double2* cs = reinterpret_cast<double2*>(c.ws + L.off_cs);
    rc = launch_prep_model(desc, c.mi, batch, branch, trunk, params, gates, cs, c.ws, c.st);
    if (rc != QHEA_OK) return rc;
    t.a = noise_args(desc, c.mi, noise, params, ham_diag, row0, batch, c.T);
    t.a.gates = gates; t.a.cs = cs; t.a.partial = reinterpret_cast<double2*>(c.ws + L.off_part);
    if (u.wide) t.mix = reinterpret_cast<double*>(c.ws + L.off_mix);
    if (u.extra) t.extra = c.ws + L.off_extra;
    return QHEA_OK;
}

// ... and their tail, behind the unit's launch (rc): row r's tiles added in tile order, mean (+ bias) and standard error
inline int traj_finish(const TrajCall& t, int rc, double* pred, double* stderr_out) {
    if (rc != QHEA_OK) return rc;
    return launch_noisy_finish(t.a.partial, t.L.tiles, t.a.B, t.c.T, t.a.bias, pred, stderr_out, t.c.st);
}

}  // namespace qhea
