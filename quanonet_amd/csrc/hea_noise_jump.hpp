// hea_noise_jump.hpp -- what the two quantum-jump trajectory units (hea_noise_device.hip, n = 2..9; hea_noise_device_wide.hip,
// n = 10..12) share beyond hea_noise_traj.hpp: the table of per-call thresholds and per-site (gamma, sqrt(1 - gamma)) in the
// workspace and the body of the prep kernel that writes it, the fenced read of a site's pair, the jump's u, the lane butterfly
// of a site's and the read-out's sums, and the body of the two entry points around a unit's kernels.  The host side of the
// noise model itself (checks, durations, the table fill) is hea_device_noise.hpp's.
#pragma once
#include <cstdint>

#include "hea_device_noise.hpp"
#include "hea_noise_traj.hpp"

namespace qhea {
namespace {

constexpr int kJumpMaxWires = 9;            // hea_noise_device.hip; n = 10..12: the state lives in LDS, hea_noise_device_wide.hip
constexpr int kWideWires = QHEA_MAX_QUBITS; // 12

template <int W>
struct JumpTable {                          // 8-byte words only: jump_tables_body copies it word by word
    unsigned long long cthr[4 * W][2];      // call c of a block's template (ENC 0..n-1, ROT n..2n-1, slot j: 2n + 2j, + 1):
                                            // (Pauli threshold, dephasing threshold)
    double gs[4][W][2];                     // [site][wire] (gamma, sqrt(1 - gamma))
    unsigned long long rthr[W][2];          // readout thresholds (01, 10) per bit
    double rd[W][2];                        // readout01, readout10 per bit
    // what the read-out of a trajectory needs of the call's arguments; the wave kernel reads it there (readout_args)
    double off, co;
    const double* diag;
    unsigned L, pauli;
};
// Named types, not aliases: they are part of every kernel's mangled name.  Their sizes are the units' TrajUnit::extra, and with
// it part of the workspace sizes the ABI answers.
struct DevTable : JumpTable<kJumpMaxWires> {};
struct WideDevTable : JumpTable<kWideWires> {};
static_assert(sizeof(DevTable) == 1472, "workspace size of qhea_model_forward_noisy_device");
static_assert(sizeof(WideDevTable) == 1952, "workspace size of qhea_model_forward_noisy_device_wide");

// (gamma, sqrt(1 - gamma)) of a site, read where the site uses it.  The addresses are loop-invariant, so without the (empty)
// fence on the offset every load of the circuit loop is hoisted in front of it and the constants are kept in scalar registers
// that spill into vector lanes (9 wires: 72 doubles); behind it the pair is one scalar load that lives for the length of its
// site.  (A fence on the pointer itself would lose its address space: flat vector loads.)
template <class Tab>
__device__ __forceinline__ double2 site_pair(const Tab* __restrict__ tab, int site, int q) {
    int fence = 0;
    asm volatile("" : "+s"(fence));
    const double* p = &tab->gs[site][q][0] + fence;
    return make_double2(p[0], p[1]);
}

// v summed over the lanes that differ in bits 0 .. BITS-1, offsets 2^(BITS-1), .., 1; every lane of a group ends with the same sum
template <int BITS>
__device__ __forceinline__ double group_sum(double v) {
    static_rfor<0, BITS>([&](auto b) { v = pair_sum<(1 << decltype(b)::value)>(v); });
    return v;
}

__device__ __forceinline__ double jump_u(unsigned w3) { return ((double)w3 + 0.5) * 0x1p-32; }

// The words of a call against entry e of the table's call template: code = the sampled Pauli (0 none; 1 .. kinds) | dephasing
// << 4, w3 = the jump's word
template <class Tab>
__device__ __forceinline__ void draw_code(const Tab* __restrict__ tab, int e, const uint4& w, unsigned kinds, unsigned& code,
                                          unsigned& w3) {
    const unsigned long long tp = tab->cthr[e][0], tz = tab->cthr[e][1];
    if ((unsigned long long)w.x < tp) code = 1u + (unsigned)(((unsigned long long)w.y * kinds) >> 32);
    if ((unsigned long long)w.z < tz) code |= 16u;
    w3 = w.w;
}

// ---- prep: the table, and expectation mode's read-out weights -------------------------------------------------------------------------

// The body of a unit's tables kernel; one workgroup of 256.  Copies the table into the workspace and, with `buf`, builds h[k] of
// expectation mode in half (n - 1) & 1 of buf[2 * 2^n]: co sum_i (bit_i(k) ? -(1 - 2 r10_i) : 1 - 2 r01_i) in the order
// i = 0..n-1, or ham_diag under the readout confusion, bit by bit: stage i writes half i & 1, h'[k] = (1 - e) h[k] + e h[k ^ 2^i]
// with e = r01_i where bit i of k is 0 and r10_i where it is 1.
template <class Tab>
__device__ __forceinline__ void jump_tables_body(const Tab& t, Tab* __restrict__ out, const double* __restrict__ diag, double co,
                                                 int n, double* __restrict__ buf) {
    constexpr int kWords = (int)(sizeof(Tab) / 8);
    static_assert(kWords <= 256, "the tables kernel copies one word per thread");
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&t);
    if ((int)threadIdx.x < kWords) reinterpret_cast<unsigned long long*>(out)[threadIdx.x] = src[threadIdx.x];
    if (!buf) return;
    const int D = 1 << n;
    if (!diag) {
        double* dst = buf + (size_t)((n - 1) & 1) * D;
        for (int k = threadIdx.x; k < D; k += 256) {
            double h = 0.0;
            for (int i = 0; i < n; ++i) h += (k >> i) & 1 ? -(1.0 - 2.0 * t.rd[i][1]) : 1.0 - 2.0 * t.rd[i][0];
            dst[k] = co * h;
        }
        return;
    }
    const double* from = diag;
    for (int i = 0; i < n; ++i) {
        double* dst = buf + (size_t)(i & 1) * D;
        for (int k = threadIdx.x; k < D; k += 256) {
            const double e = (k >> i) & 1 ? t.rd[i][1] : t.rd[i][0];
            dst[k] = (1.0 - e) * from[k] + e * from[k ^ (1 << i)];
        }
        __syncthreads();
        from = dst;
    }
}

// ---- the entry points' body (host) ------------------------------------------------------------------------------------------------------

// the value count and seed of a qhea_sampling as the qhea_noise the shared checks and layout read
inline qhea_noise sampling_as_noise(const qhea_sampling* s) {
    qhea_noise nz{};
    nz.shots = s->shots; nz.trajectories = s->trajectories; nz.seed = s->seed;
    return nz;
}

inline size_t jump_workspace_bytes(const TrajUnit& u, const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling) {
    if (!sampling) return 0;
    const qhea_noise nz = sampling_as_noise(sampling);
    return traj_workspace_bytes(u, desc, batch, &nz);
}

// qhea_model_forward_noisy_device and ..._device_wide: unit `u` (its TrajUnit::extra holds a Tab), its tables kernel and the
// launcher of its trajectory kernels
template <class Tab>
int jump_forward(const TrajUnit& u, void (*tables_kernel)(Tab, Tab*, const double*, double, int, double*),
                 int (*launch)(const NoiseArgs&, int, const Tab*, const double*, hipStream_t), const qhea_model_desc* desc,
                 int64_t row0, int64_t batch, const double* branch, const double* trunk, const double* params,
                 const double* ham_diag, const qhea_device_noise* dn, const qhea_sampling* sampling, double* pred,
                 double* stderr_out, void* workspace, size_t workspace_bytes, void* stream) {
    // the device setting is checked against the model's n before the shared checks, which read the model themselves: the first
    // reading goes into a record of its own (model_info appends to the record's block list)
    ModelInfo probe;
    int rc = model_info(desc, probe);
    if (rc != QHEA_OK) return rc;
    rc = device_noise_check(probe.n, dn);
    if (rc != QHEA_OK) return rc;
    if (!sampling) return QHEA_EINVAL;
    const qhea_noise nz = sampling_as_noise(sampling);
    TrajCall t;
    rc = traj_open(u, desc, row0, batch, branch, trunk, params, ham_diag, &nz, pred, workspace, workspace_bytes, stream, t);
    if (rc != QHEA_OK || t.c.empty) return rc;
    const int n = t.c.mi.n;
    NoiseArgs& a = t.a;
    a.L = jump_calls(n, t.c.mi.nb, t.c.mi.ld);                           // shot mode continues from call C
    Tab tb{};
    bool any;
    fill_jump_table(n, dn, tb, any);
    tb.off = a.off; tb.co = a.co; tb.diag = ham_diag; tb.L = a.L; tb.pauli = (unsigned)a.pauli;
    a.thr1 = any ? 1 : 0;                                                // an ideal setting draws nothing
    Tab* tab = reinterpret_cast<Tab*>(t.extra);
    const bool expect = !a.shots;
    hipLaunchKernelGGL(tables_kernel, dim3(1), dim3(256), 0, t.c.st, tb, tab, ham_diag, a.co, n,
                       expect ? t.mix : static_cast<double*>(nullptr));
    if (hipGetLastError() != hipSuccess) return QHEA_ELAUNCH;
    const double* hd = expect ? t.mix + ((size_t)((n - 1) & 1) << n) : nullptr;
    return traj_finish(t, launch(a, n, tab, hd, t.c.st), pred, stderr_out);
}

}  // namespace
}  // namespace qhea
