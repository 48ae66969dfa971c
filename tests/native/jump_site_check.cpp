// The host-callable arithmetic the quantum-jump gradient at n = 10..12 adds (quanonet_amd/csrc/hea_noise_jump_lds.hpp), run on the
// host: wire_reads_one (the stored-bit predicate of a site, which the reverse walk and the re-walk apply with the recorded
// polarity) and pack_words / unpack_words (a segment's record).  For n = 10, 11, 12 and every site of a sub-layer:
//   the predicate  for all 2^n amplitudes k = thread_part(t) | j << A of the pass that holds the site and both polarities it is
//                  the wire's logical bit -- basis state k of the pre-ring labels pushed through CNOT(c = i + 1 -> t = i) for the
//                  slots i = 0..j of a ring site, through nothing for a rotation site -- XOR the frame's X bit;
//   the pass       a rotation site's wire is one of the pass's own gate qubits [Q0, Q1);
//   the words      a record with any of the 36 site bits, both frames and the rescale bit comes back unchanged.
// Prints one line "checked <cases> failed <failures>"; exit status 0 iff no failure.
#include <cstdio>

#include "hea_noise_jump_lds.hpp"

using namespace qhea;

static long cases = 0, failures = 0;

static void expect(bool ok, const char* what, int n, int idx) {
    ++cases;
    if (!ok) {
        ++failures;
        if (failures <= 10) std::printf("FAIL %s n=%d site=%d\n", what, n, idx);
    }
}

// logical basis state of pre-ring label k behind the CNOT slots 0..last
template <int N>
static int pushed(int k, int last) {
    for (int i = 0; i <= last; ++i) k ^= ((k >> ((i + 1) % N)) & 1) << i;
    return k;
}

template <int N, int A, int MASK>
static bool predicate_is(int wire, int last_slot) {
    constexpr int T = 1 << (N - kLG), M = 1 << kLG;
    for (int t = 0; t < T; ++t) {
        const int tp = thread_part<A, kLG>(t);
        for (int j = 0; j < M; ++j) {
            const int k = tp | (j << A);
            const int bit = (pushed<N>(k, last_slot) >> wire) & 1;
            for (int xq = 0; xq < 2; ++xq)
                if (wire_reads_one<A, MASK>(tp, xq, j) != ((bit ^ xq) != 0)) return false;
        }
    }
    return true;
}

template <int N, int P, int Q>
static void rotation_site() {
    using PS = Pass<N, P, kLG>;
    if constexpr (Q < PS::Q1) {
        expect(predicate_is<N, PS::A, (1 << Q)>(Q, -1), "rotation", N, Q);
        rotation_site<N, P, Q + 1>();
    }
}
template <int N, int P = 0>
static void rotation_sites() {
    if constexpr (P < LCfg<N, kLG>::NP) {
        using PS = Pass<N, P, kLG>;
        static_assert(PS::Q0 >= PS::A && PS::Q1 <= PS::A + kLG, "a pass holds its gate qubits");
        rotation_site<N, P, PS::Q0>();
        rotation_sites<N, P + 1>();
    }
}

template <int N, int J = 0>
static void ring_sites() {
    if constexpr (J < N) {
        constexpr int A = Pass<N, LCfg<N, kLG>::NP - 1, kLG>::A;
        expect(predicate_is<N, A, ring_site_mask<N, J, true>()>(J, J), "TGT", N, N + 2 * J);
        expect(predicate_is<N, A, ring_site_mask<N, J, false>()>((J + 1) % N, J), "CTL", N, N + 2 * J + 1);
        ring_sites<N, J + 1>();
    }
}

static void words() {
    for (int idx = 0; idx < 36; ++idx)
        for (int r = 0; r < 2; ++r) {
            SegWords v{};
            v.fired = 1ull << idx; v.pol = (1ull << idx) | 1ull | (1ull << 35); v.px = 0xABC ^ idx; v.z = 0xFFF ^ (idx << 3);
            v.rescaled = r != 0;
            unsigned w[6];
            pack_words(v, w);
            const SegWords u = unpack_words(w);
            expect(u.fired == v.fired && u.pol == v.pol && u.px == v.px && u.z == v.z && u.rescaled == v.rescaled, "words", r, idx);
        }
    SegWords all{};
    all.fired = (1ull << 36) - 1; all.pol = (1ull << 36) - 1; all.px = 4095; all.z = 4095; all.rescaled = false;
    unsigned w[6];
    pack_words(all, w);
    const SegWords u = unpack_words(w);
    expect(u.fired == all.fired && u.pol == all.pol && !u.rescaled, "words full", 0, 36);
}

int main() {
    rotation_sites<10>(); ring_sites<10>();
    rotation_sites<11>(); ring_sites<11>();
    rotation_sites<12>(); ring_sites<12>();
    words();
    std::printf("checked %ld failed %ld\n", cases, failures);
    return failures == 0 ? 0 : 1;
}
