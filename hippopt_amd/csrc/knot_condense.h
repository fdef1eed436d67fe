// knot_condense.h — the CONDENSED block top of the preconditioner of knot_ldl.h (hipnlp.hip hipnlp_kkt_condensed_factor_kernel; the test-only
// CPU emulation tests/kkt_condensed_emu runs the same expressions from the pattern itself, in another element order).  Where d_c > 0 the
// bottom block of K = [[H + diag d_x, J^T], [J, -diag d_c]] can be eliminated instead of approximated:
//
//     C = H + diag d_x + J^T diag(1 / d_c) J,        In(K) = (0, m, 0) + In(C)        (Haynsworth)
//
// C is block tridiagonal by knot.  Its diagonal block B_k = H_k + diag d_x,k + J_k^T diag(1 / d_c) J_k needs only J_k, the column block of
// knot k: the one contiguous run of jac g the knot owns.  B_k has order 189 and is factored where H_k + d_x,k is factored today; the
// stored record has knot_ldl.h's format, so APPLY and the MINRES launches are knot_ldl.h's, unchanged.  The off-diagonal blocks of C are
// NOT formed: M stays block diagonal.
//
// ASSEMBLY: knot_ldl.h's assembly of H_k + d_x,k (every word +0.0, the stored entries, the diagonal rounded once), then every element
// (r, c), r >= c, takes ONE fused multiply-add per row i of g that has an entry in both columns r and c of the block, the rows in ASCENDING
// GLOBAL ROW INDEX:
//     s_i = 1 / d_c,i correctly rounded                                                       (kc_scale)
//     acc = fma(a_ir, a_ic * s_i, acc)        the product a_ic * s_i rounded once             (kc_term)
// One writer and one chain per element: no atomics, the same bits in every launch, at every batch position, in both orders of jac g.
// The pairs are found by a merge of the two columns' lists (kc_element): KnotCondenseTables lists the entries of a block in (column, row)
// order with the RANK of each entry's row among the rows that touch the block, ranks ascending with the global row at every knot.
//
// STATUS: a d_c,i that is not a finite number > 0 makes s_i the NaN of pl_nan().  A knot whose block is touched by such a row gets
// KL_NONFINITE without a factorisation: NaN in every word of factor, e and o, inertia (0, 0, 0) — as for block data that is not finite.
//
// THE DIAGONAL BESIDE IT, written by the same launch (with it (minv_top, minv_bottom) alone is a condensed diagonal preconditioner):
//     minv_bottom_i = s_i                                               by the row's owner (minres_owned): NaN for a bad d_c,i
//     minv_top_j    = 1 / max(|B_k,jj|, floor)                          of the ASSEMBLED diagonal, whatever the knot's status    (kc_top)
//     minv_top_g    = 1 / max(|d_x,g + sum_i J_ig^2 s_i|, floor)        the six globals, by the last knot: acc = d_x,g (+0.0 without
//                                                                       d_x), then kc_term(acc, J_ig, J_ig, s_i) in ascending row
// A value that is not finite passes through as NaN (precond_reciprocal).  The six globals' block of C is diagonal in every layout seen;
// its off-diagonal is not looked at here.
//
// WHAT THE INERTIA OF B_k PROVES: every B_k is a principal submatrix of C, so ONE negative (or zero) eigenvalue in one B_k proves that C
// is not positive definite, i.e. that K does NOT have the inertia (n, m, 0).  All B_k positive definite proves NOTHING about K: the
// off-diagonal blocks of C are not looked at.  A periodicity coupling of the Hessian pattern stays outside every block, as in knot_ldl.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "knot_hess_layout.h"
#include "knot_kkt_precond.h"
#include "knot_ldl.h"

namespace hipnlp {

constexpr int KC_ENT_MAX = 1620, KC_ROW_MAX = 439;         // entries of a column block / rows of g touching it, at most: beyond, refused
constexpr int KC_ENT_CAP = 1624, KC_ROW_CAP = 440;         // ... as the device stages them
constexpr int KC_COL_WORDS = 192;                          // column c: the entries cbeg[c] .. cbeg[c + 1]
static_assert(KC_ENT_MAX <= KC_ENT_CAP && KC_ROW_MAX <= KC_ROW_CAP && KL_N + 1 <= KC_COL_WORDS && KC_ENT_CAP < 65536 && KC_ENT_CAP <= LG_ENT_CAP, "condensation tables");

// The device tables (kc_build_tables), per block variant (first / interior / last knot).
struct alignas(16) KnotCondenseTables {
    uint16_t cbeg[3][KC_COL_WORDS];        // the entries of column c in (column, row) order: cbeg[c] .. cbeg[c + 1]
    uint16_t pos[3][KC_ENT_CAP];           // entry e: its position in the knot's block of the jac run
    uint16_t rank[3][KC_ENT_CAP];          // entry e: the rank of its row among the rows touching the block (ascending global row)
    int32_t row_a[3][KC_ROW_CAP];          // the row of rank q at knot k is row_a + row_b k   (G_NONE behind the last)
    int32_t row_b[3][KC_ROW_CAP];
    int32_t nent[3], nrows[3];
    int32_t gbeg[NXG + 2];                 // the horizon-global run: the entries of global g are gbeg[g] .. gbeg[g + 1], ascending row
    int32_t gpos[JP_GLOB_CAP], grow[JP_GLOB_CAP];   // ... position in the global run, row of g
};

// ---- the expressions ---------------------------------------------------------------------------------------------------------------------
HD double kc_scale(double dc) { return (dc > 0.0 && minres_finite(dc)) ? minres_div(1.0, dc) : pl_nan(); }
HD bool kc_scale_good(double s) { return s == s; }
HD double kc_term(double acc, double a_ir, double a_ic, double s) { return fm_fma(a_ir, a_ic * s, acc); }
HD double kc_top(double diag, double floor) { return precond_reciprocal(diag, floor); }

// One element (r, c) of the block: acc the assembled H_rc (+ d_x on the diagonal); [rb, re) / [cb, ce) the entries of columns r / c;
// rank(e), val(e) of entry e, scale(q) of the row of rank q, wherever the caller keeps them.  At most (re - rb) + (ce - cb) steps.
template <class Rank, class Val, class Scale> HD double kc_element(double acc, int rb, int re, int cb, int ce, const Rank& rank, const Val& val, const Scale& scale) {
    int p = rb, q = cb;
    while (p < re && q < ce) {
        const int rp = rank(p), rq = rank(q);
        if (rp == rq) { acc = kc_term(acc, val(p), val(q), scale(rp)); ++p; ++q; }
        else if (rp < rq) ++p;
        else ++q;
    }
    return acc;
}

// ---- what the entry point refuses before anything is launched (nullptr: nothing) ---------------------------------------------------------------
inline const char* kc_factor_call_error(bool hess, bool jac, bool dc, double floor, bool factor, bool pivots, bool e, bool o, bool inertia, bool status, bool minv_top,
                                        bool minv_bottom) {
    if (!jac) return "jac_values_dev is required";
    if (!dc) return "dc_dev is required: the condensed block eliminates the bottom block, which needs d_c > 0";
    if (const char* r = kl_factor_call_error(hess, floor, factor, pivots, e, o, inertia, status)) return r;
    if (!minv_top || !minv_bottom) return "minv_top_dev and minv_bottom_dev are required";
    return nullptr;
}

// ---- the tables: derived at a representative knot of every variant from the Lagrangian-gradient directory (the (column, row) order of a
// block whatever the jac order), then VERIFIED against the pattern at every knot.  Returns false with the reason in err.
inline bool kc_build_tables(const Layout& L, KnotCondenseTables& t, std::string& err) {
    std::memset(&t, 0, sizeof(KnotCondenseTables));
    for (int v = 0; v < 3; ++v) for (int q = 0; q < KC_ROW_CAP; ++q) t.row_a[v][q] = G_NONE;
    if (!L.jprod_ok) { err = L.jprod_error; return false; }
    const int N = L.N, krep[3] = {0, 1, N - 1};
    for (int v = 0; v < 3; ++v) {
        if (v == VAR_INTERIOR && N < 3) continue;
        const std::vector<LgradEntry>& ent = L.lg_ent[v];
        const int ne = int(ent.size()), k0 = krep[v];
        if (ne != L.nnz_v[v] || int(L.jt_pos[v].size()) != ne || int(L.lg_cbeg[v].size()) != NXK + 1) { err = "internal: condensation: the column directory is not the block"; return false; }
        // the rows touching the block, by ascending global row at the representative knot
        std::vector<std::pair<long, std::pair<int32_t, int32_t>>> rows;
        for (const LgradEntry& e : ent) rows.push_back({long(e.row_a) + long(e.row_b) * k0, {e.row_a, e.row_b}});
        std::sort(rows.begin(), rows.end());
        rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        const int nr = int(rows.size());
        if (ne > KC_ENT_MAX || nr > KC_ROW_MAX) {
            err = "a knot block of jac g has " + std::to_string(ne) + " entries in " + std::to_string(nr) + " rows: more than the condensed block factorisation stages (" +
                  std::to_string(KC_ENT_MAX) + " / " + std::to_string(KC_ROW_MAX) + ")";
            return false;
        }
        for (int q = 0; q + 1 < nr; ++q) if (rows[size_t(q)].first == rows[size_t(q) + 1].first) { err = "internal: condensation: two row families meet at one row"; return false; }
        t.nent[v] = ne; t.nrows[v] = nr;
        for (int q = 0; q < nr; ++q) { t.row_a[v][q] = rows[size_t(q)].second.first; t.row_b[v][q] = rows[size_t(q)].second.second; }
        for (int c = 0; c < KC_COL_WORDS; ++c) t.cbeg[v][c] = uint16_t(L.lg_cbeg[v][size_t(c < NXK ? c : NXK)]);
        for (int e = 0; e < ne; ++e) {
            const std::pair<long, std::pair<int32_t, int32_t>> key{long(ent[size_t(e)].row_a) + long(ent[size_t(e)].row_b) * k0, {ent[size_t(e)].row_a, ent[size_t(e)].row_b}};
            t.rank[v][e] = uint16_t(std::lower_bound(rows.begin(), rows.end(), key) - rows.begin());
            t.pos[v][e] = uint16_t(L.jt_pos[v][size_t(e)]);
        }
        // every knot of the variant: the ranks ascend with the global row, every column's ranks ascend, every entry is where the pattern has it
        for (int k = 0; k < N; ++k) {
            if (L.variant_of(k) != v) continue;
            auto row_at = [&](int q) { return long(t.row_a[v][q]) + long(t.row_b[v][q]) * k; };
            for (int q = 0; q < nr; ++q)
                if (row_at(q) < 0 || row_at(q) >= L.m || (q > 0 && row_at(q - 1) >= row_at(q))) { err = "internal: condensation: knot " + std::to_string(k) + " is not like its representative (rows)"; return false; }
            std::vector<unsigned char> seen(size_t(ne), 0);
            for (int c = 0; c < NXK; ++c)
                for (int e = t.cbeg[v][c]; e < t.cbeg[v][c + 1]; ++e) {
                    const int p = t.pos[v][e];
                    const long at = L.jac_base(k) + p;
                    if (e >= ne || p >= ne || seen[size_t(p)] || ent[size_t(e)].col != c || (e > t.cbeg[v][c] && t.rank[v][e - 1] >= t.rank[v][e]) ||
                        L.jcol[size_t(at)] != NXK * k + c || L.irow[size_t(at)] != row_at(t.rank[v][e])) {
                        err = "internal: condensation: knot " + std::to_string(k) + " is not like its representative (entries)";
                        return false;
                    }
                    seen[size_t(p)] = 1;
                }
            if (t.cbeg[v][0] != 0 || t.cbeg[v][NXK] != ne) { err = "internal: condensation: the column directory does not cover the block"; return false; }
        }
    }
    // the horizon-global run
    const int ng = int(L.lg_glob.size());
    if (ng > JP_GLOB_CAP || int(L.jt_gpos.size()) != ng || int(L.lg_gcbeg.size()) != NXG + 1 || L.lg_gcbeg[NXG] != ng) { err = "internal: condensation: the horizon-global run"; return false; }
    for (int g = 0; g <= NXG; ++g) t.gbeg[g] = L.lg_gcbeg[size_t(g)];
    t.gbeg[NXG + 1] = ng;
    for (int g = 0; g < NXG; ++g)
        for (int e = t.gbeg[g]; e < t.gbeg[g + 1]; ++e) {
            const LgradEntry& w = L.lg_glob[size_t(e)];
            const int p = L.jt_gpos[size_t(e)];
            if (w.col != g || w.row_b != 0 || p < 0 || p >= ng || L.irow[size_t(L.jac_glob_base + p)] != w.row_a || L.jcol[size_t(L.jac_glob_base + p)] != NXK * N + g ||
                w.row_a < 0 || w.row_a >= L.m || (e > t.gbeg[g] && L.lg_glob[size_t(e) - 1].row_a >= w.row_a)) {
                err = "internal: condensation: the horizon-global run is not where the pattern has it";
                return false;
            }
            t.gpos[e] = p; t.grow[e] = w.row_a;
        }
    return true;
}

}  // namespace hipnlp
