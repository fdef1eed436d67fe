// TEST-ONLY CPU emulation of hipnlp_kkt_times_kernel (hipnlp.hip): per knot the staging of the workgroup, then the sums of knot_jprod.h and
// knot_hvp.h over the directories Layout::build and HessLayout::build record and the two combining expressions of knot_kkt.h — the same
// headers, the same table words the device reads — on value runs the caller supplies.  No knot program runs here.
// It is NOT part of the product: libhipnlp.so does not contain it.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../hippopt_amd/csrc/knot_hess_layout.h"
#include "../../hippopt_amd/csrc/knot_kkt.h"
#include "../../hippopt_amd/csrc/layout.h"
#include "../values_stage_emu.h"

using namespace hipnlp;

struct kktemu_handle {
    hipnlp_desc d;
    KinTables kt;
    Layout L;
    HessLayout HL;
    JprodTables T;
};

extern "C" {

kktemu_handle* kktemu_create(const hipnlp_desc* desc, char* err, int errlen) {
    kktemu_handle* h = new kktemu_handle();
    h->d = *desc;
    std::string e;
    if (Layout::make_kin_tables(desc->model, h->kt, e)) Layout::fill_terrain_tops(h->kt, desc->settings.terrain, desc->settings.n_terrain_steps, desc->settings.terrain_steps);
    if (e.empty() && !h->L.build(desc->settings, h->kt, (desc->flags & HIPNLP_FLAG_DETECT_SIMPLE_BOUNDS) != 0, (desc->flags & HIPNLP_FLAG_JAC_VARYING_FIRST) != 0)) e = h->L.error;
    if (e.empty() && !h->HL.build(desc->settings, h->kt)) e = h->HL.error;
    if (e.empty() && !h->L.lgrad_ok) e = h->L.lgrad_error;
    if (e.empty() && !h->L.jprod_ok) e = h->L.jprod_error;
    if (e.empty() && !h->HL.hvp_ok) e = h->HL.hvp_error;
    if (!e.empty()) {
        std::strncpy(err, e.c_str(), size_t(errlen - 1));
        delete h;
        return nullptr;
    }
    h->L.fill_jprod_tables(h->T);
    return h;
}
void kktemu_destroy(kktemu_handle* h) { delete h; }
void kktemu_dims(const kktemu_handle* h, int* n, int* m, int* nnz, long* nnz_h) { *n = h->L.n; *m = h->L.m; *nnz = h->L.nnz; *nnz_h = h->HL.nnz; }
void kktemu_sparsity(const kktemu_handle* h, int* irow, int* jcol) {
    for (int i = 0; i < h->L.nnz; ++i) { irow[i] = h->L.irow[size_t(i)]; jcol[i] = h->L.jcol[size_t(i)]; }
}
void kktemu_hess_sparsity(const kktemu_handle* h, int* irow, int* jcol) { h->HL.pattern(irow, jcol); }

// top [n] = (H + diag dx) v + J^T w, bottom [m] = J v - diag(dc) w from the value runs hess [nnz_h] and jac [nnz]; dx / dc may be null;
// top_writes [n] / bottom_writes [m] count the stores
void kktemu_times(const kktemu_handle* h, const double* hess, const double* jac, const double* dx, const double* dc, const double* v, const double* w, double* top, double* bottom,
                  int* top_writes, int* bottom_writes) {
    const Layout& L = h->L;
    const HessLayout& HL = h->HL;
    const JprodTables& T = h->T;
    const int N = L.N;
    std::vector<double> js(JP_VALUES), vs(JP_V_WORDS), ls(LG_LAM_CAP), jg(LG_ENT_CAP + 16);
    std::vector<int32_t> lw(LG_ENT_CAP + 16);
    auto store_top = [&](long i, double y) { top[i] = y; top_writes[i]++; };
    for (int k = 0; k < N; ++k) {
        const int pv = L.pair_variant_of(k), bv = L.variant_of(k), first = k == 0, last = k == N - 1;
        // phase 1 staging, as the workgroup does it (tests/values_stage_emu.h)
        values_stage_emu::stage_jac_rows(L, T, jac, k, js.data());
        values_stage_emu::stage_records_of(v, k, N, vs.data());
        values_stage_emu::stage_column_words(L, bv, last, lw.data());
        std::fill(ls.begin(), ls.end(), 0.0);
        std::fill(jg.begin(), jg.end(), 0.0);
        for (size_t q = 0; q < L.lg_rows[bv].size(); ++q) ls[q] = w[L.lg_rows[bv][q].first + L.lg_rows[bv][q].second * k];
        if (last)   // the horizon-global run for the last knot's global columns: addressed from LG_ENT_CAP on
            for (size_t i = 0; i < L.jperm_glob.size(); ++i) jg[LG_ENT_CAP + i] = jac[L.jac_glob_base + long(i)];
        // the owned rows of J v, and bottom
        for (int q = 0; q < JP_ROW_CAP; ++q) {
            if (T.row_a[pv][q] == G_NONE) continue;
            const long r = long(T.row_a[pv][q]) + long(T.row_b[pv][q]) * k;
            const double jv = jprod_row_staged(T.rdir[pv][q], T.word[pv], js.data(), vs.data());
            bottom[r] = kkt_bottom(dc != nullptr, dc ? dc[r] : 0.0, dc ? w[r] : 0.0, jv);
            bottom_writes[r]++;
        }
        // phase 2: the Hessian block by position, the touches in the order of the table
        const bool ends_coupled = HL.n_couple > 0 && (first || last);
        const double* blk = hess + HL.knot_base(k);
        const double* vo = v + long(NXK) * (first ? N - 1 : 0);
        auto val = [&](int e) { return blk[HL.hv_touch[size_t(e)].pos]; };
        auto vec = [&](int e) { return vs[size_t(HL.hv_touch[size_t(e)].other)]; };
        for (int c = 0; c < NXK; ++c) {
            const double jt = jprod_column_staged(false, 0.0, 0.0, L.lg_cbeg[bv][size_t(c)], L.lg_cbeg[bv][size_t(c) + 1], lw.data(), ls.data(), js.data());
            const bool coupled = ends_coupled && HL.hv_couple[size_t(c)] >= 0;
            const double cpl = coupled ? hess[HL.couple_base() + HL.hv_couple[size_t(c)]] : 0.0;
            const double hv = hvp_row(HL.hv_beg[size_t(c)], HL.hv_beg[size_t(c) + 1], val, vec, coupled, cpl, coupled ? vo[c] : 0.0);
            const long i = long(NXK) * k + c;
            store_top(i, kkt_top(dx != nullptr, dx ? dx[i] : 0.0, vs[size_t(c)], hv, jt));
        }
        if (last)   // no entry of the Hessian touches the horizon-global variables
            for (int c = 0; c < NXG; ++c) {
                const double jt = jprod_column_staged(false, 0.0, 0.0, LG_ENT_CAP + L.lg_gcbeg[size_t(c)], LG_ENT_CAP + L.lg_gcbeg[size_t(c) + 1], lw.data(), ls.data(), jg.data());
                const long i = long(NXK) * N + c;
                store_top(i, kkt_top(dx != nullptr, dx ? dx[i] : 0.0, vs[size_t(JP_V_GLOB + c)], 0.0, jt));
            }
    }
}

}  // extern "C"
