// The index and sign arithmetic of store_framed and load_framed (quanonet_amd/csrc/hea_lds.hpp), run on the host: thread_part,
// phys, ring_dst, ring_pull, group_slot, frame_local and frame_neg are __host__ __device__, so this is the arithmetic the device
// runs.  For one (N, LG, A, RING) and a frame (x, z), over all 2^N amplitudes k = thread_part(t) | j << A:
//   bounds     every slot the scatter writes lies in [0, 2^N) and no two amplitudes share one;
//   the frame  the slot phys(m) then holds, up to one sign common to all m, (-1)^parity(m & z) v[ring^-1(m ^ x)] -- the Pauli
//              string X^x Z^z behind the ring (RING) or behind nothing;
//   the mirror the gather through the same frame returns v[k] to every k, up to one sign common to all k.
// Prints one line "checked <cases> failed <failures>"; exit status 0 iff no failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hea_lds.hpp"

using namespace qhea;

static int parity(int v) { return __builtin_popcount((unsigned)v) & 1; }

template <int N, int LG, int A, bool RING>
static int check(int x, int z) {
    constexpr int D = 1 << N, M = 1 << LG, T = 1 << (N - LG);
    const int px = phys<LG>(x), zp = RING ? ring_pull<N>(z) : z;
    std::vector<int> slot_of(D, -1), sign_at(D, 0);            // per LDS slot: the amplitude stored there and its sign
    for (int t = 0; t < T; ++t) {
        const int tp = thread_part<A, LG>(t);
        const int base = RING ? phys<LG>(ring_dst<N>(tp)) : phys<LG>(tp);
        const int sb = __builtin_popcount((unsigned)(tp & zp)), zl = frame_local<A, LG>(zp);
        for (int j = 0; j < M; ++j) {
            const int slot = base ^ px ^ (RING ? phys<LG>(ring_dst<N>(j << A)) : phys<LG>(j << A));
            if (slot < 0 || slot >= D || slot_of[slot] != -1) return 1;
            slot_of[slot] = tp | (j << A);
            sign_at[slot] = frame_neg(sb, zl, j) ? -1 : 1;
        }
    }
    // the frame: slot phys(m) holds amplitude k with ring(k) = m ^ x (or k = m ^ x), signed by parity(m & z) up to one sign
    int common = 0;
    for (int m = 0; m < D; ++m) {
        const int k = slot_of[phys<LG>(m)];
        if (k < 0 || (RING ? ring_dst<N>(k) : k) != (m ^ x)) return 2;
        const int s = sign_at[phys<LG>(m)] * (parity(m & z) ? -1 : 1);
        if (common == 0) common = s;
        if (s != common) return 3;
    }
    // the mirror: thread t's gather of local amplitude j reads the slot it stored to and applies the same sign
    common = 0;
    for (int t = 0; t < T; ++t) {
        const int tp = thread_part<A, LG>(t);
        const int base = RING ? phys<LG>(ring_dst<N>(tp)) : phys<LG>(tp);
        const int sb = __builtin_popcount((unsigned)(tp & zp)), zl = frame_local<A, LG>(zp);
        for (int j = 0; j < M; ++j) {
            const int slot = base ^ px ^ group_slot<N, A, RING, LG>(j);
            if (slot_of[slot] != (tp | (j << A))) return 4;
            const int s = sign_at[slot] * (frame_neg(sb, zl, j) ? -1 : 1);
            if (common == 0) common = s;
            if (s != common) return 5;
        }
    }
    return 0;
}

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned next_u32() {                                   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (unsigned)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static long cases = 0, failures = 0;

template <int N, int LG, int A>
static void run_pass(int pairs) {
    for (int i = 0; i < pairs; ++i) {
        // the first pairs are the corners: no frame, X only, Z only, everything
        const int full = (1 << N) - 1;
        const int x = i == 0 ? 0 : i == 1 ? full : i == 2 ? 0 : i == 3 ? full : (int)(next_u32() & full);
        const int z = i == 0 ? 0 : i == 1 ? 0 : i == 2 ? full : i == 3 ? full : (int)(next_u32() & full);
        for (int ring = 0; ring < 2; ++ring) {
            const int rc = ring ? check<N, LG, A, true>(x, z) : check<N, LG, A, false>(x, z);
            ++cases;
            if (rc) {
                ++failures;
                if (failures <= 10) std::printf("FAIL n=%d LG=%d A=%d ring=%d x=%d z=%d code=%d\n", N, LG, A, ring, x, z, rc);
            }
        }
    }
}

template <int N, int LG, int P = 0>
static void run_layout(int pairs) {
    if constexpr (P < LCfg<N, LG>::NP) {
        run_pass<N, LG, Pass<N, P, LG>::A>(pairs);
        run_layout<N, LG, P + 1>(pairs);
    }
}

int main(int argc, char** argv) {
    const int pairs = argc > 1 ? std::atoi(argv[1]) : 300;
    // the layouts in use: the sampled-trajectory gradient kernel (3 gate qubits per pass at n = 10, 11, 4 at n = 12) and the
    // forward trajectory kernels (4 at every n)
    run_layout<10, 3>(pairs); run_layout<11, 3>(pairs); run_layout<12, 3>(pairs);
    run_layout<10, 4>(pairs); run_layout<11, 4>(pairs); run_layout<12, 4>(pairs);
    std::printf("checked %ld failed %ld\n", cases, failures);
    return failures == 0 ? 0 : 1;
}
