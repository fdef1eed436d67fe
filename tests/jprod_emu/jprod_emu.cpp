// TEST-ONLY CPU emulation of hipnlp_jac_times_kernel and hipnlp_jac_transpose_times_kernel (hipnlp.hip): the sums of knot_jprod.h over
// the row and column directories Layout::build records — the same header, the same table words the device reads, the same staging —
// on a value run the caller supplies.  No knot program runs here.
// It is NOT part of the product: libhipnlp.so does not contain it.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../hippopt_amd/csrc/layout.h"
#include "../values_stage_emu.h"

using namespace hipnlp;

struct jpemu_handle {
    hipnlp_desc d;
    KinTables kt;
    Layout L;
    JprodTables T;
};

extern "C" {

jpemu_handle* jpemu_create(const hipnlp_desc* desc, char* err, int errlen) {
    jpemu_handle* h = new jpemu_handle();
    h->d = *desc;
    std::string e;
    if (Layout::make_kin_tables(desc->model, h->kt, e)) Layout::fill_terrain_tops(h->kt, desc->settings.terrain, desc->settings.n_terrain_steps, desc->settings.terrain_steps);
    if (e.empty() && !h->L.build(desc->settings, h->kt, (desc->flags & HIPNLP_FLAG_DETECT_SIMPLE_BOUNDS) != 0, (desc->flags & HIPNLP_FLAG_JAC_VARYING_FIRST) != 0)) e = h->L.error;
    if (e.empty() && !h->L.jprod_ok) e = h->L.jprod_error;
    if (!e.empty()) {
        std::strncpy(err, e.c_str(), size_t(errlen - 1));
        delete h;
        return nullptr;
    }
    h->L.fill_jprod_tables(h->T);
    return h;
}
void jpemu_destroy(jpemu_handle* h) { delete h; }
void jpemu_dims(const jpemu_handle* h, int* n, int* m, int* nnz) { *n = h->L.n; *m = h->L.m; *nnz = h->L.nnz; }
void jpemu_sparsity(const jpemu_handle* h, int* irow, int* jcol) {
    for (int i = 0; i < h->L.nnz; ++i) { irow[i] = h->L.irow[size_t(i)]; jcol[i] = h->L.jcol[size_t(i)]; }
}
// counts per pair variant: owned rows, entries; then entries of the first block the last knot stages, horizon-global entries, and per
// block variant the entries and the multipliers   ([4] [4] [1] [1] [3] [3])
void jpemu_counts(const jpemu_handle* h, int* out) {
    const Layout& L = h->L;
    for (int pv = 0; pv < PV_COUNT; ++pv) { out[pv] = int(L.jp_rows[pv].size()); out[4 + pv] = int(L.jp_ent[pv].size()); }
    out[8] = int(L.jp_other.size()); out[9] = int(L.jperm_glob.size());
    for (int v = 0; v < 3; ++v) { out[10 + v] = L.nnz_v[v]; out[13 + v] = int(L.lg_rows[v].size()); }
}

// index in the pattern of the staged value `pos` of knot k (from the DEVICE table words: what the kernel would read)
static long pattern_index(const jpemu_handle* h, int k, int pos) {
    const Layout& L = h->L;
    if (pos >= JP_POS_GLOB) return k == 0 ? long(L.jac_glob_base) + (pos - JP_POS_GLOB) : -1;
    if (pos >= JP_POS_OTHER) return k == L.N - 1 && h->T.other[pos - JP_POS_OTHER] >= 0 ? L.jac_base(0) + h->T.other[pos - JP_POS_OTHER] : -1;
    if (pos >= JP_POS_PRED) return k > 0 && pos - JP_POS_PRED < L.nnz_v[L.variant_of(k - 1)] ? L.jac_base(k - 1) + (pos - JP_POS_PRED) : -1;
    return pos < L.nnz_v[L.variant_of(k)] ? L.jac_base(k) + pos : -1;
}
// variable of the NLP behind the staged element `var` of v at knot k
static long variable_index(const jpemu_handle* h, int k, int var) {
    const int N = h->L.N;
    if (var >= JP_V_GLOB) return long(NXK) * N + (var - JP_V_GLOB);
    if (var >= JP_V_OTHER) return var - JP_V_OTHER;
    if (var >= JP_V_PRED) return long(NXK) * (k - 1) + (var - JP_V_PRED);
    return long(NXK) * k + var;
}

// The row directory expanded over the horizon, read back from the device table words: owners[r] counts the knots that own row r; entry
// t of the directory (returns how many; at most cap) is pattern entry ent_idx[t], listed under row ent_row[t] of knot ent_knot[t] with
// the variable ent_var[t] of v.  Entries of one row are consecutive, in the order of the sum.
long jpemu_row_directory(const jpemu_handle* h, int* owners, long cap, long* ent_idx, int* ent_row, int* ent_knot, long* ent_var) {
    const Layout& L = h->L;
    for (int r = 0; r < L.m; ++r) owners[r] = 0;
    long t = 0;
    for (int k = 0; k < L.N; ++k) {
        const int pv = L.pair_variant_of(k);
        for (int q = 0; q < JP_ROW_CAP; ++q) {
            if (h->T.row_a[pv][q] == G_NONE) continue;
            const int r = h->T.row_a[pv][q] + h->T.row_b[pv][q] * k;
            if (r >= 0 && r < L.m) owners[r]++;
            const int beg = h->T.rdir[pv][q] & JP_POS_MASK, end = beg + (h->T.rdir[pv][q] >> JP_POS_BITS);
            for (int e = beg; e < end; ++e, ++t) {
                if (t >= cap) return -1;
                const int32_t w = h->T.word[pv][e];
                ent_idx[t] = pattern_index(h, k, w & JP_POS_MASK);
                ent_row[t] = r; ent_knot[t] = k;
                ent_var[t] = variable_index(h, k, w >> JP_POS_BITS);
            }
        }
    }
    return t;
}
// The column directory expanded over the horizon: entry t is pattern entry ent_idx[t], listed under column ent_col[t] with the multiplier
// of row ent_row[t].  Entries of one column are consecutive, in the order of the sum.
long jpemu_col_directory(const jpemu_handle* h, long cap, long* ent_idx, int* ent_col, int* ent_row) {
    const Layout& L = h->L;
    long t = 0;
    for (int k = 0; k < L.N; ++k) {
        const int v = L.variant_of(k);
        for (size_t e = 0; e < L.lg_ent[v].size(); ++e, ++t) {
            if (t >= cap) return -1;
            const auto& rr = L.lg_rows[v][size_t(L.lg_ent[v][e].lam)];
            ent_idx[t] = L.jac_base(k) + L.jt_pos[v][e];
            ent_col[t] = NXK * k + L.lg_ent[v][e].col;
            ent_row[t] = rr.first + rr.second * k;
        }
    }
    for (size_t e = 0; e < L.lg_glob.size(); ++e, ++t) {
        if (t >= cap) return -1;
        const auto& rr = L.lg_rows[VAR_LAST][size_t(L.lg_glob[e].lam)];
        ent_idx[t] = long(L.jac_glob_base) + L.jt_gpos[e];
        ent_col[t] = NXK * L.N + L.lg_glob[e].col;
        ent_row[t] = rr.first + rr.second * (L.N - 1);
    }
    return t;
}

// hipnlp_jac_times_kernel + the reduction of the per-knot partials: jv [m] (or null) = J v, *dot (or null; needs grad) = grad . v, from
// the value run values [nnz]; jv_writes [m] / dot_writes [1] count the stores
void jpemu_jac_times(const jpemu_handle* h, const double* values, const double* grad, const double* v, double* jv, double* dot, int* jv_writes, int* dot_writes) {
    const Layout& L = h->L;
    const JprodTables& T = h->T;
    const int N = L.N;
    std::vector<double> part(static_cast<size_t>(N), 0.0);
    std::vector<double> js(JP_VALUES), vs(JP_V_WORDS);
    for (int k = 0; k < N; ++k) {
        const int pv = L.pair_variant_of(k);
        // staging, as the workgroup does it (tests/values_stage_emu.h)
        values_stage_emu::stage_jac_rows(L, T, values, k, js.data());
        values_stage_emu::stage_records_of(v, k, N, vs.data());
        if (jv)
            for (int q = 0; q < JP_ROW_CAP; ++q) {
                if (T.row_a[pv][q] == G_NONE) continue;
                const long r = long(T.row_a[pv][q]) + long(T.row_b[pv][q]) * k;
                jv[r] = jprod_row_staged(T.rdir[pv][q], T.word[pv], js.data(), vs.data());
                if (jv_writes) jv_writes[r]++;
            }
        if (dot && grad) {
            double prod[JP_WG];
            for (int t = 0; t < JP_WG; ++t) prod[t] = t < NXK ? jprod_dot_product(grad[long(NXK) * k + t], vs[size_t(t)]) : 0.0;
            part[size_t(k)] = jprod_dot_tree(prod);
        }
    }
    if (dot && grad) {
        double acc = 0.0;
        for (int k = 0; k < N; ++k) acc += part[size_t(k)];
        *dot = acc;
        if (dot_writes) dot_writes[0]++;
    }
}

// hipnlp_jac_transpose_times_kernel: out [n] = sigma grad + J^T lambda (grad null: J^T lambda) from the value run values [nnz]
void jpemu_jac_transpose_times(const jpemu_handle* h, const double* values, const double* grad, double sigma, const double* lambda, double* out, int* writes) {
    const Layout& L = h->L;
    const int N = L.N;
    std::vector<double> js(LG_ENT_CAP + 16), ls(LG_LAM_CAP);
    std::vector<int32_t> w(LG_ENT_CAP + 16);
    auto store = [&](long i, double y) { out[i] = y; if (writes) writes[i]++; };
    for (int k = 0; k < N; ++k) {
        const int v = L.variant_of(k), last = k == N - 1;
        std::fill(js.begin(), js.end(), 0.0);
        std::fill(ls.begin(), ls.end(), 0.0);
        for (int i = 0; i < LG_ENT_CAP; ++i) js[size_t(i)] = i < L.nnz_v[v] ? values[L.jac_base(k) + i] : 0.0;
        for (size_t q = 0; q < L.lg_rows[v].size(); ++q) ls[q] = lambda[L.lg_rows[v][q].first + L.lg_rows[v][q].second * k];
        values_stage_emu::stage_column_words(L, v, last, w.data());
        if (last)
            for (size_t i = 0; i < L.jperm_glob.size(); ++i) js[LG_ENT_CAP + i] = values[L.jac_glob_base + long(i)];
        for (int c = 0; c < NXK; ++c)
            store(long(NXK) * k + c, jprod_column_staged(grad != nullptr, sigma, grad ? grad[long(NXK) * k + c] : 0.0, L.lg_cbeg[v][size_t(c)], L.lg_cbeg[v][size_t(c) + 1], w.data(), ls.data(), js.data()));
        if (last)   // the global variables carry no cost
            for (int c = 0; c < NXG; ++c)
                store(long(NXK) * N + c, jprod_column_staged(grad != nullptr, sigma, 0.0, LG_ENT_CAP + L.lg_gcbeg[size_t(c)], LG_ENT_CAP + L.lg_gcbeg[size_t(c) + 1], w.data(), ls.data(), js.data()));
    }
}

}  // extern "C"
