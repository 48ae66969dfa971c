// Stand-alone host check of model_info() (quanonet_amd/csrc/hea_model.hpp): over a grid of model descriptors, the Shape it
// builds by appending the model's one or two runs must be member for member the Shape make_shape() builds from the explicit
// per-block arrays, and a QuanONet with equal trunk and branch sub-layer counts must come out as one run.  Not a pytest.
// Build and run from quanonet_amd/csrc after `make` (the other objects come from build/obj):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I../../include -I. -Xarch_host -fsanitize=address,undefined \
//       -x hip ../../tests/native/model_info_check.cpp hea_api.hip -x none $(ls ../../build/obj/*.o | grep -v hea_api) -o model_info_check
#include <cstdio>
#include <vector>

#include "hea_model.hpp"

using namespace qhea;

static bool same(const Shape& a, const Shape& b) {
    if (a.E != b.E || a.blk != b.blk || a.nblocks != b.nblocks || a.fast_ld != b.fast_ld || a.runs.nruns != b.runs.nruns) return false;
    for (int k = 0; k < kMaxRuns; ++k)
        if (a.runs.count[k] != b.runs.count[k] || a.runs.enc[k] != b.runs.enc[k] || a.runs.ld[k] != b.runs.ld[k]) return false;
    return true;
}

int main() {
    const int vals[] = {0, 1, 2, 3, 5};
    long checked = 0, bad = 0;
    for (int model = 0; model < 2; ++model)
        for (int n = 2; n <= 12; ++n)
            for (int a : vals) for (int b : vals) for (int c : vals) for (int d : vals)
                for (int trainable = 0; trainable < 2; ++trainable) {
                    if (model == QHEA_MODEL_HEAQNN && (c || d)) continue;
                    qhea_model_desc desc{};
                    desc.model = model; desc.n_qubits = n;
                    desc.net[0] = a; desc.net[1] = b; desc.net[2] = c; desc.net[3] = d;
                    desc.branch_in = 3; desc.trunk_in = 2; desc.trainable_freq = trainable; desc.ham_pauli = QHEA_PAULI_Z;
                    ModelInfo mi;
                    const int rc = model_info(&desc, mi);
                    // the block list written out: QuanONet = net[2] trunk blocks of net[3] sub-layers, then net[0] branch
                    // blocks of net[1]; HEAQNN = net[0] blocks of net[1]
                    std::vector<int32_t> enc, ld;
                    if (model == QHEA_MODEL_QUANONET) for (int i = 0; i < c; ++i) { enc.push_back(n); ld.push_back(d); }
                    for (int i = 0; i < a; ++i) { enc.push_back(n); ld.push_back(b); }
                    Shape ref;
                    const int rc_ref = make_shape(n, (int)enc.size(), enc.data(), ld.data(), ref);
                    ++checked;
                    bool ok = rc == rc_ref && rc == QHEA_OK && same(mi.sh, ref);
                    const int want_nb[2] = {model == QHEA_MODEL_QUANONET ? c : a, model == QHEA_MODEL_QUANONET ? a : 0};
                    const int want_ld[2] = {model == QHEA_MODEL_QUANONET ? d : b, model == QHEA_MODEL_QUANONET ? b : 0};
                    for (int g = 0; g < 2; ++g) ok = ok && mi.nb[g] == want_nb[g] && mi.ld[g] == want_ld[g];
                    if (model == QHEA_MODEL_QUANONET && a > 0 && c > 0 && b == d) ok = ok && mi.sh.runs.nruns == 1 && mi.sh.runs.count[0] == a + c;
                    if (!ok) {
                        ++bad;
                        printf("MISMATCH model=%d n=%d net=(%d,%d,%d,%d) rc=%d/%d nruns=%d/%d\n", model, n, a, b, c, d, rc, rc_ref,
                               mi.sh.runs.nruns, ref.runs.nruns);
                    }
                }
    printf("model_info vs make_shape: %ld descriptors, %ld mismatches\n", checked, bad);
    return bad ? 1 : 0;
}
