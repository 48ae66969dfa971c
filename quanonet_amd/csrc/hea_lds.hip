// hea_lds.hip -- workgroup-resident variant of the HEA simulator for the largest qubit counts (n = 10..12).
//
// The wave-resident kernels (hea_device.hpp, built for n <= 9) keep 2^(n-6) amplitudes per lane in VGPRs; with psi
// and lambda live that exceeds the 256 architectural VGPRs for n >= 11 (backward) / n = 12 (forward) and the compiler
// spills to scratch.  Here ONE workgroup of 2^(n-4) threads owns one sample; the state(s) rest in LDS
// (n = 12: 64 KB per state, psi + lambda = 128 of the CU's 160 KB) and every thread works on 16 (forward) or 8
// (backward) amplitudes at a time in registers:
//
//   * a gate layer (the n fused SU(2) gates of a sub-layer) is ceil(n/LG) passes, LG = 4 or 3; pass p loads, per
//     thread, the 2^LG amplitudes that differ in index bits A..A+LG-1 (A = LG p, or n-LG for a ragged last pass),
//     applies the gates of those qubits as in-register 2x2 updates and stores them back -- one LDS round trip
//     of the state per LG gates;
//   * a block's RX encodings are folded, per sample, into the fused gates of its first sub-layer
//     (U RX(theta) is again an SU(2) matrix), so they cost no layer of their own; their gradient is
//     n . (X,Y,Z) of that sub-layer's inner products with n = axis of U X U^dagger (rotated_x_axis);
//     only encodings beyond n per block, or a block without sub-layers, still run as RX layers;
//   * the CNOT ring is a permutation of the basis index that is linear over GF(2), so it costs no pass of
//     its own: the last pass of a forward sub-layer scatters its amplitudes to ring(k), the first pass of a
//     reverse sub-layer gathers from ring(k); per amplitude that is ONE xor with a compile-time constant
//     on top of a per-thread base computed once per kernel;
//   * LDS index swizzle (phys): for every pass the 16-byte accesses of 16 neighbouring lanes fall into 16
//     different bank quads (a thread's 16 amplitudes would otherwise sit 256 B apart for A = 0).
//
// Same circuit, same fused SU(2) table, same adjoint recipe (X,Y,Z inner products taken after the fused gate,
// mapped to the three angles in reduce_kernel) as the wave-resident kernels.  Bound by fp64 FMA issue
// (16 FMAs per amplitude pair and gate; 44 in the reverse sweep) plus the LDS round trip of each pass, which
// the barriers keep from overlapping with the arithmetic when only one workgroup fits a CU (backward, n = 12).
// Measured, cfg 5 (n = 12, Net40-2-20-2, B = 1024): forward 1.90 ms, forward + backward 8.47 ms (the previous
// gate-pair-per-pass LDS kernels: 6.6 / 21.8 ms).
#include "hea_lds.hpp"
#include "hea_qsweep.hpp"

namespace qhea {

namespace {

// the pass layout (LCfg, Pass, Bases), phys, ring_dst and load_group / apply_group / store_group: hea_lds.hpp

// merge_rx / rotated_x_axis (the RX fold) are shared with the wave-resident kernels: hea_device.hpp

// Per-sample gate coefficients of a layer (folded RX) are computed ONCE per layer by threads 0..n-1 into a
// small LDS table and read back (broadcast) right before use.  Computing them inline in every thread made
// the compiler keep all of a layer's merged gates live and spill ~1500 registers (measured: 10x slower).
template <int N, class F>
__device__ __forceinline__ void set_gates(double4* gtab, F f) {
    if (threadIdx.x < N) gtab[threadIdx.x] = f((int)threadIdx.x);
    __syncthreads();
}
// One forward gate layer.  gate(q, u) fills u and returns whether qubit q has a gate (wave-uniform).
// RING: the last pass scatters through the CNOT ring.
template <int N, int LG, bool RING, class G>
__device__ __forceinline__ void fwd_layer(double2* s, const Bases<N, LG>& bs, G gate) {
    constexpr int NP = LCfg<N, LG>::NP;
    static_for<0, NP>([&](auto p) {
        constexpr int P = decltype(p)::value;
        using PS = Pass<N, P, LG>;
        c2 v[1 << LG];
        load_group<N, PS::A, false, LG>(s, bs.plain[P], v);
        static_for<PS::Q0, PS::Q1>([&](auto q) {
            constexpr int Q = decltype(q)::value;
            double4 u;
            if (gate(Q, u)) apply_group<Q - PS::A, LG>(v, u);
        });
        if constexpr (RING && P == NP - 1) {
            __syncthreads();                               // every thread holds its amplitudes: safe to permute
            store_group<N, PS::A, true, LG>(s, bs.ring, v);
            __syncthreads();
        } else {
            store_group<N, PS::A, false, LG>(s, bs.plain[P], v);
            // the next pass: P + 1, or pass 0 of the following layer
            pass_sync<wave_local_passes<N, LG, P, (P + 1 < NP ? P + 1 : 0)>()>();
        }
    });
}

// inner / inner_x and the reverse layer on psi and lambda (bwd_layer): hea_lds.hpp, shared with hea_noise_grad_lds.hip

__device__ __forceinline__ double4 gate_u(const char* gates, int n, int sub, int q) {   // base variant of gate (sub,q)
    return *reinterpret_cast<const double4*>(gates + ((long)(sub + 1) * n + q) * kGateBytes);
}

template <int N>
__device__ __forceinline__ double ham_w(int k, double off, double co, const double* __restrict__ diag) {
    return diag ? diag[k] : off + co * (double)(N - 2 * (int)__popc((unsigned)k));
}

// sum of one double per thread over the workgroup (fixed order), result in every thread
template <int N, int LG>
__device__ __forceinline__ double block_sum(double v, double* scratch) {
    double t[1] = {v};
    lane_reduce<1, 6>(t, threadIdx.x & 63);
    if constexpr (LCfg<N, LG>::NW == 1) return t[0];
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = t[0];
    __syncthreads();
    double tot = scratch[0];
#pragma unroll
    for (int w = 1; w < LCfg<N, LG>::NW; ++w) tot += scratch[w];
    __syncthreads();                                       // scratch is reused by the caller
    return tot;
}

// readout-basis change on every qubit (see basis_change in hea_device.hpp): X -> RY(-pi/2), Y -> RX(+pi/2)
template <int N, int LG>
__device__ __forceinline__ void basis_lds(double2* s, const Bases<N, LG>& bs, int pauli, bool dag) {
    if (pauli == 0) return;
    const double r = 0.70710678118654752440, sr = dag ? -r : r;
    const double4 uc = pauli == 1 ? make_double4(r, 0.0, sr, 0.0) : make_double4(r, 0.0, 0.0, -sr);
    fwd_layer<N, LG, false>(s, bs, [&](int, double4& u) { u = uc; return true; });
}

// MEM: a sweep member's block counts (run_count, hea_device.hpp) instead of the run table's
template <int N, int LG, bool MEM = false>
__device__ __forceinline__ void forward_lds(double2* psi, double4* gtab, const Bases<N, LG>& bs, const Runs& runs,
                                            const double2* __restrict__ cs_b, const char* __restrict__ gates,
                                            DepthCounts dc = DepthCounts{0, 0}) {
    using L = LCfg<N, LG>;
#pragma unroll
    for (int j = 0; j < L::M; ++j) {
        const int p = threadIdx.x + j * L::T;
        psi[p] = make_double2(p == 0 ? 1.0 : 0.0, 0.0);              // |0..0>: phys(0) = 0
    }
    __syncthreads();
    int col = 0, sub = 0;
    for (int ri = 0; ri < runs.nruns; ++ri) {
        const int ne = runs.enc[ri], nld = runs.ld[ri];
        for (int rep = 0; rep < run_count<MEM>(runs, ri, dc); ++rep) {
            // RX(x[col+j]) on wire j % n, n wires per layer; the last layer is folded into the first sub-layer
            const int nchunks = (ne + N - 1) / N;
            const int nsep = (nld > 0 && ne > 0) ? nchunks - 1 : nchunks;
            for (int ch = 0; ch < nsep; ++ch) {
                const int j0 = ch * N;
                const int m = (ne - j0) < N ? (ne - j0) : N;
                const double2* c = cs_b + col + j0;
                fwd_layer<N, LG, false>(psi, bs, [&](int q, double4& u) {
                    if (q >= m) return false;
                    u = rx_su2(c[q]);
                    return true;
                });
            }
            if (nsep < nchunks) {
                const int j0 = nsep * N;
                const int m = ne - j0;
                const double2* c = cs_b + col + j0;
                set_gates<N>(gtab, [&](int q) {
                    return merge_rx(gate_u(gates, N, sub, q), q < m ? c[q] : make_double2(1.0, 0.0));
                });
                fwd_layer<N, LG, true>(psi, bs, [&](int q, double4& u) { u = gtab[q]; return true; });
                ++sub;
            }
            col += ne;
            for (int l = (nsep < nchunks) ? 1 : 0; l < nld; ++l, ++sub)
                fwd_layer<N, LG, true>(psi, bs, [&](int q, double4& u) { u = gate_u(gates, N, sub, q); return true; });
        }
    }
}

}  // namespace

template <int N>
__global__ __launch_bounds__((LCfg<N, kFwdLG>::T)) void lds_fwd_kernel(Runs runs, long B, int E, const double2* __restrict__ cs,
                                                             const char* __restrict__ gates, double off, double co,
                                                             const double* __restrict__ diag, int pauli,
                                                             double* __restrict__ out, double* __restrict__ state_out,
                                                             const double* __restrict__ bias) {
    constexpr int LG = kFwdLG;
    using L = LCfg<N, LG>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* psi = reinterpret_cast<double2*>(smem);
    double* scratch = reinterpret_cast<double*>(smem + L::STATE_BYTES);
    double4* gtab = reinterpret_cast<double4*>(scratch + L::NW * 64);
    const long b = blockIdx.x;
    Bases<N, LG> bs;
    bs.init(threadIdx.x);
    forward_lds<N, LG>(psi, gtab, bs, runs, cs + b * E, gates);
    if (state_out) {
#pragma unroll
        for (int j = 0; j < L::M; ++j) {
            const int k = threadIdx.x + j * L::T;
            reinterpret_cast<double2*>(state_out)[(b << N) + k] = psi[phys<LG>(k)];
        }
    }
    basis_lds<N, LG>(psi, bs, pauli, false);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < L::M; ++j) {
        const int k = threadIdx.x + j * L::T;
        const double2 a = psi[phys<LG>(k)];
        acc += ham_w<N>(k, off, co, diag) * (a.x * a.x + a.y * a.y);
    }
    const double tot = block_sum<N, LG>(acc, scratch);
    if (threadIdx.x == 0) out[b] = tot + (bias ? bias[0] : 0.0);
}

// Backward: one row of `partial` per sample ([B][blk][KW]); grad_x written directly.
// DA: empty for the single-model kernel; one DepthArgs (depth sweeps, ensembles and sweeps: member = blockIdx.y) or one
// QubitArgs (qubit sweeps: member = work-list entry blockIdx.y) for the member instantiations, whose prologue moves the
// pointers to the member's and sets its E, blk, read-out and block counts, as bwd_kernel's does (hea_device.hpp).  The sample
// is blockIdx.x in both forms.
template <int N, class... DA>
__global__ __launch_bounds__((LCfg<N, kBwdLG>::T)) void lds_bwd_kernel(Runs runs, long B, int E, int blk,
                                                             const double2* __restrict__ cs,
                                                             const char* __restrict__ gates, double off, double co,
                                                             const double* __restrict__ diag, int pauli,
                                                             const double* __restrict__ g,
                                                             const double* __restrict__ state_in,
                                                             const double* __restrict__ y,
                                                             const double* __restrict__ bias, double inv_bt,
                                                             double* __restrict__ out, double* __restrict__ grad_x,
                                                             double* __restrict__ partial, DA... da) {
    constexpr int LG = kBwdLG;
    using L = LCfg<N, LG>;
    constexpr int KW = L::KW;
    constexpr bool MEM = sizeof...(DA) != 0;
    DepthCounts dc{0, 0};
    if constexpr (MEM) {        // the member's counts, shape, read-out and pointers (the launch's are member 0's)
        const auto d = (da, ...);
        const auto mr = d.rec();
        dc.c0 = mr->depth[0]; dc.c1 = mr->depth[1];
        E = N * (dc.c0 + dc.c1);
        blk = dc.c0 * runs.ld[0] + dc.c1 * runs.ld[1];
        off = mr->off; co = mr->co; diag = mr->diag; pauli = mr->pauli;
        const long wsb = d.ws_bytes();
        cs = reinterpret_cast<const double2*>(reinterpret_cast<const char*>(cs) + wsb);
        gates += wsb;
        out = reinterpret_cast<double*>(reinterpret_cast<char*>(out) + wsb);
        grad_x = reinterpret_cast<double*>(reinterpret_cast<char*>(grad_x) + wsb);
        partial = reinterpret_cast<double*>(reinterpret_cast<char*>(partial) + wsb);
        y = reinterpret_cast<const double*>(reinterpret_cast<const char*>(y) + d.row_bytes());
        if (bias) bias = reinterpret_cast<const double*>(reinterpret_cast<const char*>(bias) + d.param_bytes());
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* psi = reinterpret_cast<double2*>(smem);
    double2* lam = psi + L::DIM;
    double* scratch = reinterpret_cast<double*>(smem + 2 * L::STATE_BYTES);        // [NW][64]
    double4* gtab = reinterpret_cast<double4*>(scratch + L::NW * 64);
    const long b = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double2* __restrict__ cs_b = cs + b * E;
    Bases<N, LG> bs;
    bs.init(threadIdx.x);

    if (state_in) {
#pragma unroll
        for (int j = 0; j < L::M; ++j) {
            const int k = threadIdx.x + j * L::T;
            psi[phys<LG>(k)] = reinterpret_cast<const double2*>(state_in)[(b << N) + k];
        }
        __syncthreads();
    } else {
        forward_lds<N, LG, MEM>(psi, gtab, bs, runs, cs_b, gates, dc);
    }
    basis_lds<N, LG>(psi, bs, pauli, false);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < L::M; ++j) {
        const int k = threadIdx.x + j * L::T;
        const double2 a = psi[phys<LG>(k)];
        acc += ham_w<N>(k, off, co, diag) * (a.x * a.x + a.y * a.y);
    }
    const double pred = block_sum<N, LG>(acc, scratch) + (bias ? bias[0] : 0.0);
    if (out && threadIdx.x == 0) out[b] = pred;
    const double gb = y ? 2.0 * (pred - y[b]) * inv_bt : g[b];
#pragma unroll
    for (int j = 0; j < L::M; ++j) {
        const int k = threadIdx.x + j * L::T;
        const double2 a = psi[phys<LG>(k)];
        const double h = gb * ham_w<N>(k, off, co, diag);
        lam[phys<LG>(k)] = make_double2(h * a.x, h * a.y);
    }
    __syncthreads();
    basis_lds<N, LG>(psi, bs, pauli, true);
    basis_lds<N, LG>(lam, bs, pauli, true);

    double* __restrict__ part_b = partial + b * (long)blk * KW;
    int col = E, sub = blk;
    for (int ri = runs.nruns - 1; ri >= 0; --ri) {
        const int ne = runs.enc[ri], nld = runs.ld[ri];
        const int nchunks = (ne + N - 1) / N;
        for (int rep = 0; rep < run_count<MEM>(runs, ri, dc); ++rep) {
            const int nsep = (nld > 0 && ne > 0) ? nchunks - 1 : nchunks;      // see forward_lds
            const int m_merged = nsep < nchunks ? ne - nsep * N : 0;
            col -= ne;
            for (int l = nld - 1; l >= 0; --l) {
                --sub;
                const int mm = l == 0 ? m_merged : 0;           // encodings folded into this sub-layer's gates
                const double2* c = cs_b + col + nsep * N;
                double xyz[KW];
#pragma unroll
                for (int i = 0; i < KW; ++i) xyz[i] = 0.0;
                set_gates<N>(gtab, [&](int q) {
                    return dagger(merge_rx(gate_u(gates, N, sub, q), q < mm ? c[q] : make_double2(1.0, 0.0)));
                });
                bwd_layer<N, LG, true, true>(psi, lam, bs, [&](int q, double4& u) { u = gtab[q]; return true; }, xyz);
                // workgroup sum of the 3n per-thread values: wave butterfly, then the waves through LDS
                lane_reduce<KW, 6>(xyz, lane);               // lane i holds the wave total of value i
                if (lane < KW) scratch[wv * 64 + lane] = xyz[0];
                __syncthreads();
                if (threadIdx.x < KW) {
                    double tot = scratch[threadIdx.x];
#pragma unroll
                    for (int w = 1; w < L::NW; ++w) tot += scratch[w * 64 + threadIdx.x];
                    part_b[(long)sub * KW + threadIdx.x] = tot;
                }
                if (threadIdx.x < mm) {                      // encoding gradient of the folded RX on wire threadIdx.x
                    const int q = threadIdx.x;
                    double X = 0.0, Y = 0.0, Z = 0.0;
#pragma unroll
                    for (int w = 0; w < L::NW; ++w) {
                        X += scratch[w * 64 + 3 * q]; Y += scratch[w * 64 + 3 * q + 1]; Z += scratch[w * 64 + 3 * q + 2];
                    }
                    double nx, ny, nz;
                    rotated_x_axis(gate_u(gates, N, sub, q), nx, ny, nz);
                    grad_x[b * E + col + nsep * N + q] = nx * X + ny * Y + nz * Z;
                }
                __syncthreads();
            }
            for (int ch = nsep - 1; ch >= 0; --ch) {            // remaining RX layers in reverse order
                const int j0 = ch * N;
                const int m = (ne - j0) < N ? (ne - j0) : N;
                const double2* c = cs_b + col + j0;
                double gx[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) gx[i] = 0.0;
                bwd_layer<N, LG, false, false>(psi, lam, bs, [&](int q, double4& u) {
                    if (q >= m) return false;
                    u = dagger(rx_su2(c[q]));
                    return true;
                }, gx);
                lane_reduce<16, 6>(gx, lane);                // lane l holds the wave total of value l & 15
                if constexpr (L::NW == 1) {
                    if (lane < m) grad_x[b * E + col + j0 + lane] = gx[0];
                } else {
                    if (lane < 16) scratch[wv * 64 + lane] = gx[0];
                    __syncthreads();
                    if (threadIdx.x < m) {
                        double tot = scratch[threadIdx.x];
#pragma unroll
                        for (int w = 1; w < L::NW; ++w) tot += scratch[w * 64 + threadIdx.x];
                        grad_x[b * E + col + j0 + threadIdx.x] = tot;
                    }
                    __syncthreads();
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
namespace {

template <int N>
int launch_fwd_n(long B, hipStream_t st, const FwdArgs& a) {
    using L = LCfg<N, kFwdLG>;
    constexpr size_t smem = L::STATE_BYTES + L::SCRATCH_BYTES;
    return launch_dynamic_lds(lds_fwd_kernel<N>, dim3((unsigned)B), dim3(L::T), smem, st, a.runs, a.B, a.E, a.cs, a.gates, a.off,
                              a.co, a.diag, a.pauli, a.out, a.state_out, a.bias);
}

template <int N>
int launch_bwd_n(long B, hipStream_t st, const BwdArgs& a) {
    using L = LCfg<N, kBwdLG>;
    constexpr size_t smem = 2 * L::STATE_BYTES + L::SCRATCH_BYTES;
    return launch_dynamic_lds(lds_bwd_kernel<N>, dim3((unsigned)B), dim3(L::T), smem, st, a.runs, a.B, a.E, a.blk, a.cs, a.gates,
                              a.off, a.co, a.diag, a.pauli, a.g, a.state_in, a.y, a.bias, a.inv_bt, a.out, a.grad_x, a.partial);
}

// member launches: grid (samples, members); A = DepthArgs or QubitArgs
template <int N, class A>
int launch_bwd_member_n(dim3 grid, hipStream_t st, const BwdArgs& a, const A& m) {
    using L = LCfg<N, kBwdLG>;
    constexpr size_t smem = 2 * L::STATE_BYTES + L::SCRATCH_BYTES;
    return launch_dynamic_lds(lds_bwd_kernel<N, A>, grid, dim3(L::T), smem, st, a.runs, a.B, a.E, a.blk, a.cs, a.gates, a.off, a.co,
                              a.diag, a.pauli, a.g, a.state_in, a.y, a.bias, a.inv_bt, a.out, a.grad_x, a.partial, m);
}
template <class A>
int launch_bwd_member(int n, dim3 grid, hipStream_t st, const BwdArgs& a, const A& m) {
    switch (n) {
        case 10: return launch_bwd_member_n<10>(grid, st, a, m);
        case 11: return launch_bwd_member_n<11>(grid, st, a, m);
        case 12: return launch_bwd_member_n<12>(grid, st, a, m);
        default: return QHEA_EUNSUPPORTED;
    }
}

}  // namespace

bool lds_supported(int n) { return n >= 10 && n <= 12; }

int launch_lds_bwd_depth(int n, dim3 grid, hipStream_t st, const BwdArgs& a, const DepthArgs& d) {
    return launch_bwd_member(n, grid, st, a, d);
}

int launch_lds_bwd_qubit(int n, dim3 grid, hipStream_t st, const BwdArgs& a, const QubitArgs& q) {
    return launch_bwd_member(n, grid, st, a, q);
}

int launch_lds_fwd(int n, long B, hipStream_t st, const FwdArgs& a) {
    switch (n) {
        case 10: return launch_fwd_n<10>(B, st, a);
        case 11: return launch_fwd_n<11>(B, st, a);
        case 12: return launch_fwd_n<12>(B, st, a);
        default: return QHEA_EUNSUPPORTED;
    }
}

int launch_lds_bwd(int n, long B, hipStream_t st, const BwdArgs& a) {
    switch (n) {
        case 10: return launch_bwd_n<10>(B, st, a);
        case 11: return launch_bwd_n<11>(B, st, a);
        case 12: return launch_bwd_n<12>(B, st, a);
        default: return QHEA_EUNSUPPORTED;
    }
}

}  // namespace qhea
