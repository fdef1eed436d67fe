// TEST-ONLY: the staging of a stored-values workgroup as the CPU emulations state it (tests/jprod_emu, tests/kkt_emu,
// tests/kkt_precond_emu) — from the vectors of Layout, in plain loops over every element of the staged arrays.  It is the reference the
// device staging (hippopt_amd/csrc/knot_values_stage.h) is compared against and deliberately does NOT include that header.
// It is NOT part of the product: libhipnlp.so does not contain it.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../hippopt_amd/csrc/layout.h"

namespace values_stage_emu {
using namespace hipnlp;

// js [JP_VALUES]: the own block of knot k, the predecessor's block, the entries of knot 0's block the last knot needs, the horizon-global
// run at knot 0 (zeros where a guard keeps a load from happening)
inline void stage_jac_rows(const Layout& L, const JprodTables& T, const double* values, int k, double* js) {
    const int first = k == 0, last = k == L.N - 1;
    const int nnz_own = L.nnz_v[L.variant_of(k)], nnz_pred = first ? 0 : L.nnz_v[L.variant_of(k - 1)];
    std::fill(js, js + JP_VALUES, 0.0);
    for (int i = 0; i < JP_BLOCK_CAP; ++i) {
        js[i] = i < nnz_own ? values[L.jac_base(k) + i] : 0.0;
        js[JP_POS_PRED + i] = i < nnz_pred ? values[L.jac_base(k - 1) + i] : 0.0;
    }
    for (int i = 0; i < JP_OTHER_CAP; ++i) js[JP_POS_OTHER + i] = (last && T.other[i] >= 0) ? values[L.jac_base(0) + T.other[i]] : 0.0;
    for (int i = 0; i < JP_GLOB_CAP; ++i) js[JP_POS_GLOB + i] = (first && i < int(L.jperm_glob.size())) ? values[L.jac_glob_base + i] : 0.0;
}

// rs [JP_V_WORDS]: four records in the JP_V_* arrangement — own knot, predecessor, other horizon end (last knot), the globals; zeros where
// a record does not exist.  knot(kk, i): element i of the record of knot kk; glob(i): global element i.
template <class Knot, class Glob> void stage_records(int k, int N, double* rs, const Knot& knot, const Glob& glob) {
    const int first = k == 0, last = k == N - 1;
    std::fill(rs, rs + JP_V_WORDS, 0.0);
    for (int i = 0; i < NXK; ++i) {
        rs[i] = knot(k, i);
        rs[JP_V_PRED + i] = first ? 0.0 : knot(k - 1, i);
        rs[JP_V_OTHER + i] = last ? knot(0, i) : 0.0;
    }
    for (int i = 0; i < NXG; ++i) rs[JP_V_GLOB + i] = glob(i);
}
// ... of a vector v [n]
inline void stage_records_of(const double* v, int k, int N, double* rs) {
    stage_records(k, N, rs, [&](int kk, int i) { return v[long(NXK) * kk + i]; }, [&](int i) { return v[long(NXK) * N + i]; });
}

// w [LG_ENT_CAP + 16]: the column words of a knot of block variant v — block position | multiplier position << LG_SLOT_BITS, -1 behind;
// from LG_ENT_CAP on the words of the horizon-global columns (last knot), which address their run from LG_ENT_CAP on
inline void stage_column_words(const Layout& L, int v, bool last, int32_t* w) {
    std::fill(w, w + LG_ENT_CAP + 16, int32_t(-1));
    for (size_t e = 0; e < L.lg_ent[v].size(); ++e) w[e] = int32_t(L.jt_pos[v][e] | (L.lg_ent[v][e].lam << LG_SLOT_BITS));
    if (last)
        for (size_t e = 0; e < L.lg_glob.size(); ++e) w[LG_ENT_CAP + e] = int32_t((LG_ENT_CAP + L.jt_gpos[e]) | (L.lg_glob[e].lam << LG_SLOT_BITS));
}

}  // namespace values_stage_emu
