// hea_noise_traj.hpp -- what the trajectory kernels of the noisy forward share: hea_noise.hip (n = 2..6, one amplitude per lane)
// and hea_noise_wide.hip (n = 7..12, registers or LDS).  The argument record, the Philox stream and its error codes, the Pauli
// frame bits, the checks of a qhea_noise and the finish launch that turns tile sums into a row's mean and standard error.
#pragma once
#include <cstdint>

#include "hea_noise.hpp"

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

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// values per row (T trajectories or S shots), or QHEA_EINVAL
inline int64_t noise_values(const qhea_noise* nz) {
    if (!nz) return QHEA_EINVAL;
    for (double p : {nz->p1, nz->p2, nz->readout})
        if (!(p >= 0.0 && p <= 1.0)) return QHEA_EINVAL;
    if (nz->shots < 0) return QHEA_EINVAL;
    const int64_t T = nz->shots > 0 ? nz->shots : nz->trajectories;
    if (T < 1 || T > (int64_t)0xFFFFFFFF) return QHEA_EINVAL;          // trajectory index is one 32-bit counter word
    return T;
}

inline unsigned long long threshold(double p) { return (unsigned long long)(p * 4294967296.0); }

// everything of NoiseArgs that the descriptor and the noise setting fix; the caller adds the workspace pointers
inline NoiseArgs noise_args(const qhea_model_desc* desc, const NoiseShape& ns, const qhea_noise* noise, const double* params,
                            const double* ham_diag, int64_t row0, int64_t batch, int64_t T) {
    NoiseArgs a{};
    a.diag = ham_diag;
    a.bias = ns.off_bias >= 0 ? params + ns.off_bias : nullptr;
    a.off = desc->ham_offset; a.co = desc->ham_coeff; a.q = noise->readout;
    a.thr1 = threshold(noise->p1); a.thr2 = threshold(noise->p2); a.thrq = threshold(noise->readout);
    a.B = batch; a.row0 = row0; a.T = T; a.tiles = (int)((T + kTile - 1) / kTile); a.E = ns.E; a.pauli = desc->ham_pauli;
    a.shots = noise->shots > 0 ? 1 : 0;
    unsigned locs = 0;
    for (int g = 0; g < 2; ++g) {
        a.nb[g] = ns.nb[g]; a.ld[g] = ns.ld[g];
        locs += (unsigned)ns.nb[g] * (unsigned)(ns.n + 2 * ns.n * ns.ld[g]);
    }
    a.L = locs;
    a.key0 = (unsigned)noise->seed; a.key1 = (unsigned)(noise->seed >> 32);
    return a;
}

// noisy_finish_kernel (hea_noise.hip) on `st`: row r's tiles added in tile order, mean (+ bias) and standard error
int launch_noisy_finish(const double2* partial, int tiles, int64_t B, int64_t T, const double* bias, double* pred, double* se,
                        hipStream_t st);

}  // namespace qhea
