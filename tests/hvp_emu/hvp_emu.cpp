// TEST-ONLY CPU emulation of hipnlp_knot_hvp_kernel and hipnlp_hess_times_kernel (hipnlp.hip): the Hessian program of knot_hess_body.h per
// knot (multiplier gather as in hipnlp_knot_hess_kernel), then the per-variable sums of knot_hvp.h over the touch tables
// HessLayout::build records — the same header, the same tables the device reads; and the same sums from a stored value run.
// It is NOT part of the product: libhipnlp.so does not contain it.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../hippopt_amd/csrc/knot_hess_layout.h"
#include "../../hippopt_amd/csrc/knot_hvp.h"

using namespace hipnlp;

namespace {
struct HvEm {
    static constexpr int kTerrain = -1;
    double* g;
    double* jac;
    double* hess = nullptr;
    void G(int slot, int, double v) { g[slot] = v; }
    void J(int slot, int, int, double v) { jac[slot] = v; }
    void H(int slot, int, int, double v) { hess[slot] = v; }
};
}  // namespace

struct hvemu_handle {
    hipnlp_desc d;
    KinTables kt;
    KSettings ks;
    Layout L;
    HessLayout HL;
};

extern "C" {

hvemu_handle* hvemu_create(const hipnlp_desc* desc, char* err, int errlen) {
    hvemu_handle* h = new hvemu_handle();
    h->d = *desc;
    std::string e;
    if (Layout::make_kin_tables(desc->model, h->kt, e)) Layout::fill_terrain_tops(h->kt, desc->settings.terrain, desc->settings.n_terrain_steps, desc->settings.terrain_steps);
    if (e.empty() && !h->L.build(desc->settings, h->kt, (desc->flags & HIPNLP_FLAG_DETECT_SIMPLE_BOUNDS) != 0, (desc->flags & HIPNLP_FLAG_JAC_VARYING_FIRST) != 0)) e = h->L.error;
    if (e.empty() && !h->HL.build(desc->settings, h->kt)) e = h->HL.error;
    if (e.empty() && !h->HL.hvp_ok) e = h->HL.hvp_error;
    if (!e.empty()) {
        std::strncpy(err, e.c_str(), size_t(errlen - 1));
        delete h;
        return nullptr;
    }
    h->ks = Layout::make_ksettings(desc->settings);
    return h;
}
void hvemu_destroy(hvemu_handle* h) { delete h; }
void hvemu_dims(const hvemu_handle* h, int* n, int* m, long* nnz_h, int* nnz_knot, int* n_couple, int* touches) {
    *n = h->L.n; *m = h->L.m; *nnz_h = h->HL.nnz; *nnz_knot = h->HL.nnz_knot; *n_couple = h->HL.n_couple; *touches = int(h->HL.hv_touch.size());
}
int hvemu_m_full(const hvemu_handle* h) { return h->L.m_full; }
void hvemu_lift_map(const hvemu_handle* h, int* kept_row) { h->L.kept_rows(kept_row); }
void hvemu_hess_sparsity(const hvemu_handle* h, int* irow, int* jcol) { h->HL.pattern(irow, jcol); }
// the touch tables: beg [NXK + 1], K [NXK], couple [NXK], and per touch its position in the block, its native slot and its other variable
void hvemu_tables(const hvemu_handle* h, int* beg, int* K, int* couple, int* pos, int* slot, int* other) {
    const HessLayout& HL = h->HL;
    for (int i = 0; i <= NXK; ++i) beg[i] = HL.hv_beg[size_t(i)];
    for (int i = 0; i < NXK; ++i) { K[i] = HL.hv_K[size_t(i)]; couple[i] = HL.hv_couple[size_t(i)]; }
    for (size_t e = 0; e < HL.hv_touch.size(); ++e) { pos[e] = HL.hv_touch[e].pos; slot[e] = HL.hv_touch[e].slot; other[e] = HL.hv_touch[e].other; }
}
// positions of a knot block -> native slot; coupling entries -> native slot
void hvemu_perm(const hvemu_handle* h, int* perm, int* perm_couple) {
    for (int i = 0; i < h->HL.nnz_knot; ++i) perm[i] = h->HL.perm[size_t(i)];
    for (int i = 0; i < h->HL.n_couple; ++i) perm_couple[i] = h->HL.perm_couple[size_t(i)];
}

// out [n] = H(x, sigma, lambda) v, the fused kernel's way; writes[i] (or null) counts the stores into out[i]; values (or null) [nnz_h]
// receives the value run hipnlp_eval_hess_device writes
void hvemu_hess_vec(const hvemu_handle* h, const double* x, const double* p, double sigma, const double* lambda, const double* v, double* out, int* writes,
                    double* values) {
    const Layout& L = h->L;
    const HessLayout& HL = h->HL;
    const int N = L.N;
    std::vector<double> pk(size_t(N) * PK_STRIDE);
    GParams gp;
    pack_params(p, N, pk.data(), gp);
    KnotScratch* s = new KnotScratch();
    KHessScratch* hx = new KHessScratch();
    auto store = [&](long i, double y) { out[i] = y; if (writes) writes[i]++; };
    for (int k = 0; k < N; ++k) {
        std::fill(reinterpret_cast<double*>(s), reinterpret_cast<double*>(s) + sizeof(KnotScratch) / sizeof(double), std::nan(""));
        std::fill(reinterpret_cast<double*>(hx), reinterpret_cast<double*>(hx) + sizeof(KHessScratch) / sizeof(double), std::nan(""));
        for (int i = 0; i < XPAD; ++i) { s->x[i] = 0; s->xm[i] = 0; }
        for (int i = 0; i < NXK; ++i) { s->x[i] = x[NXK * k + i]; s->xm[i] = k > 0 ? x[NXK * (k - 1) + i] : 0.0; }
        for (int i = 0; i < NPER; ++i) s->xo[i] = k == 0 ? x[NXK * (N - 1) + periodicity_row_var(i)] : (k == N - 1 ? x[periodicity_row_var(i)] : 0.0);
        for (int i = 0; i < NXG; ++i) s->xg[i] = x[NXK * N + i];
        for (int i = 0; i < PK_STRIDE; ++i) s->pk[i] = pk[size_t(k) * PK_STRIDE + i];
        const int var = L.variant_of(k);
        for (int i = 0; i < 3; ++i) {
            const int slot = gs::HDYN + 3 + i, vn = L.variant_of(k + 1);
            const int a = k + 1 < N ? L.g_a[vn][size_t(slot)] : G_NONE;
            hx->lam_next[i] = a != G_NONE ? lambda[a + L.g_b[size_t(slot)] * (k + 1)] : 0.0;
        }
        hx->sigma = sigma;
        kh_fill_far_lists(h->kt, hx->far);
        const bool first = k == 0, last = k == N - 1;
        KnotInfo ki{k, N, first, last};
        HvEm em{s->g, s->jac, hx->H};
        Ctx<HvEm> cx(*s, h->kt, h->ks, gp, ki, em);
        for (int slot = 0; slot < gs::COUNT; ++slot) { const int a = L.g_a[var][size_t(slot)]; s->g[slot] = a != G_NONE ? lambda[a + L.g_b[size_t(slot)] * k] : 0.0; }
        KHCtx<HvEm> hcx{cx, *hx, s->g};
#define HOST_KIN(w, fn, nt) for (int t_ = 0; t_ < (nt); ++t_) fn(cx, t_);
#define HOST_RH(w, fn, nt) for (int t_ = 0; t_ < (nt); ++t_) fn(hcx, t_);
        HIPNLP_KNOT_HESS_PROGRAM(HOST_KIN, HOST_RH, )
#undef HOST_KIN
#undef HOST_RH
        if (values) {
            for (int i = 0; i < HL.nnz_knot; ++i) values[HL.knot_base(k) + i] = hx->H[HL.perm[size_t(i)]];
            if (last) for (int i = 0; i < HL.n_couple; ++i) values[HL.couple_base() + i] = hx->H[HL.perm_couple[size_t(i)]];
        }
        // the program has ended: one variable after the other, values by native slot from the staging, v from this knot's record
        const double cpl = kh_percouple_value(sigma, h->ks.periodicity_weight);
        const bool ends_coupled = HL.n_couple > 0 && (first || last);
        const double* vk = v + long(NXK) * k;
        const double* vo = v + long(NXK) * (first ? N - 1 : 0);
        auto val = [&](int e) { return hx->H[HL.hv_touch[size_t(e)].slot]; };
        auto vec = [&](int e) { return vk[HL.hv_touch[size_t(e)].other]; };
        for (int i = 0; i < NXK; ++i) {
            const bool coupled = ends_coupled && HL.hv_couple[size_t(i)] >= 0;
            store(long(NXK) * k + i, hvp_row(HL.hv_beg[size_t(i)], HL.hv_beg[size_t(i) + 1], val, vec, coupled, cpl, coupled ? vo[i] : 0.0));
        }
        if (last) for (int i = 0; i < NXG; ++i) store(long(NXK) * N + i, 0.0);
    }
    delete hx;
    delete s;
}

// out [n] = H v from a value run [nnz_h] (hipnlp_hess_times_kernel): values by block position, coupling values from the end of the run
void hvemu_hess_times(const hvemu_handle* h, const double* values, const double* v, double* out, int* writes) {
    const HessLayout& HL = h->HL;
    const int N = h->L.N;
    auto store = [&](long i, double y) { out[i] = y; if (writes) writes[i]++; };
    for (int k = 0; k < N; ++k) {
        const bool first = k == 0, last = k == N - 1;
        const bool ends_coupled = HL.n_couple > 0 && (first || last);
        const double* blk = values + HL.knot_base(k);
        const double* vk = v + long(NXK) * k;
        const double* vo = v + long(NXK) * (first ? N - 1 : 0);
        auto val = [&](int e) { return blk[HL.hv_touch[size_t(e)].pos]; };
        auto vec = [&](int e) { return vk[HL.hv_touch[size_t(e)].other]; };
        for (int i = 0; i < NXK; ++i) {
            const bool coupled = ends_coupled && HL.hv_couple[size_t(i)] >= 0;
            const double cpl = coupled ? values[HL.couple_base() + HL.hv_couple[size_t(i)]] : 0.0;
            store(long(NXK) * k + i, hvp_row(HL.hv_beg[size_t(i)], HL.hv_beg[size_t(i) + 1], val, vec, coupled, cpl, coupled ? vo[i] : 0.0));
        }
        if (last) for (int i = 0; i < NXG; ++i) store(long(NXK) * N + i, 0.0);
    }
}

}  // extern "C"
