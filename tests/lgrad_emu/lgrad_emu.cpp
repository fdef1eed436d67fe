// TEST-ONLY CPU emulation of hipnlp_knot_lgrad_kernel (hipnlp.hip): the knot program of knot_body.h on the compact scratch of the
// device's four-wave kernels, the multipliers of the rows a block touches staged in the g staging once the program has ended, then the
// per-column reduction of knot_lgrad.h over the tables Layout::build records — the same header, the same tables the device reads.
// It is NOT part of the product: libhipnlp.so does not contain it.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../hippopt_amd/csrc/layout.h"

using namespace hipnlp;

namespace {
// the device emitter's staging (DevEm of the non-VARY four-wave kernel): every entry of jac g, constants included (no JC member)
struct LgEm {
    static constexpr int kTerrain = -1;
    using Scratch = KnotScratchT<LAYOUT_COMPACT>;
    double* g;
    double* jac;
    void G(int slot, int, double v) { g[slot] = v; }
    void J(int slot, int, int, double v) { jac[slot] = v; }
};
}  // namespace

struct lgemu_handle {
    hipnlp_desc d;
    KinTables kt;
    KSettings ks;
    Layout L;
};

extern "C" {

lgemu_handle* lgemu_create(const hipnlp_desc* desc, char* err, int errlen) {
    lgemu_handle* h = new lgemu_handle();
    h->d = *desc;
    std::string e;
    if (Layout::make_kin_tables(desc->model, h->kt, e)) Layout::fill_terrain_tops(h->kt, desc->settings.terrain, desc->settings.n_terrain_steps, desc->settings.terrain_steps);
    if (!e.empty() || !h->L.build(desc->settings, h->kt, (desc->flags & HIPNLP_FLAG_DETECT_SIMPLE_BOUNDS) != 0, (desc->flags & HIPNLP_FLAG_JAC_VARYING_FIRST) != 0)) {
        if (e.empty()) e = h->L.error;
        std::strncpy(err, e.c_str(), size_t(errlen - 1));
        delete h;
        return nullptr;
    }
    h->ks = Layout::make_ksettings(desc->settings);
    return h;
}
void lgemu_destroy(lgemu_handle* h) { delete h; }
void lgemu_dims(const lgemu_handle* h, int* n, int* m, int* nnz) { *n = h->L.n; *m = h->L.m; *nnz = h->L.nnz; }
void lgemu_sparsity(const lgemu_handle* h, int* irow, int* jcol) {
    std::memcpy(irow, h->L.irow.data(), sizeof(int) * h->L.irow.size());
    std::memcpy(jcol, h->L.jcol.data(), sizeof(int) * h->L.jcol.size());
}
// 1: the tables fit the device kernel's staging; 0: they do not (the message in err)
int lgemu_tables_ok(const lgemu_handle* h, char* err, int errlen) {
    std::strncpy(err, h->L.lgrad_error.c_str(), size_t(errlen - 1));
    return h->L.lgrad_ok ? 1 : 0;
}
int lgemu_m_full(const lgemu_handle* h) { return h->L.m_full; }
void lgemu_lift_map(const lgemu_handle* h, int* kept_row) { h->L.kept_rows(kept_row); }
// entries and multiplier rows of a first / interior / last block, entries of the horizon-global columns
void lgemu_table_sizes(const lgemu_handle* h, int* entries /*[3]*/, int* rows /*[3]*/, int* glob) {
    for (int v = 0; v < 3; ++v) { entries[v] = int(h->L.lg_ent[v].size()); rows[v] = int(h->L.lg_rows[v].size()); }
    *glob = int(h->L.lg_glob.size());
}

// out [n] = sigma grad f(x) + J(x)^T lambda (lambda [m] of this layout); writes[i] (or null) counts the stores into out[i].  Returns the
// number of multiplier rows outside [0, m) the tables asked for (0), -1 when the tables do not fit the kernel.
int lgemu_lagrangian_grad(const lgemu_handle* h, const double* x, const double* p, double sigma, const double* lambda, double* out, int* writes) {
    const Layout& L = h->L;
    const int N = L.N;
    if (!L.lgrad_ok) return -1;   // (the device call answers HIPNLP_E_UNSUPPORTED)
    int bad_rows = 0;
    std::vector<double> pk(size_t(N) * PK_STRIDE);
    GParams gp;
    pack_params(p, N, pk.data(), gp);
    using S = KnotScratchT<LAYOUT_COMPACT>;
    S* s = new S();
    auto store = [&](long i, double v) { out[i] = v; if (writes) writes[i]++; };
    for (int k = 0; k < N; ++k) {
        std::fill(reinterpret_cast<double*>(s), reinterpret_cast<double*>(s) + sizeof(S) / sizeof(double), std::nan(""));
        for (int i = 0; i < XPAD; ++i) { s->x[i] = 0; s->xm[i] = 0; }
        for (int i = 0; i < NXK; ++i) { s->x[i] = x[NXK * k + i]; s->xm[i] = k > 0 ? x[NXK * (k - 1) + i] : 0.0; }
        for (int i = 0; i < NPER; ++i) s->xo[i] = k == 0 ? x[NXK * (N - 1) + periodicity_row_var(i)] : (k == N - 1 ? x[periodicity_row_var(i)] : 0.0);
        for (int i = 0; i < NXG; ++i) s->xg[i] = x[NXK * N + i];
        for (int i = 0; i < 8 - NXG; ++i) s->xg[NXG + i] = 0.0;
        for (int i = 0; i < PK_STRIDE; ++i) s->pk[i] = pk[size_t(k) * PK_STRIDE + i];
        KnotInfo ki{k, N, k == 0, k == N - 1};
        LgEm em{s->g, s->jac};
        Ctx<LgEm> cx(*s, static_cast<const KinLite&>(h->kt), h->ks, static_cast<const GParamsLite&>(gp), ki, em, &h->kt, &gp);
#define HOST_R(w4, w8, fn, nt) for (int t_ = 0; t_ < (nt); ++t_) fn(cx, t_);
        HIPNLP_KNOT_PROGRAM(HOST_R, )
#undef HOST_R
        // the program has ended: the multipliers of the rows the block touches go where the device stages them, then every column is summed
        const int v = L.variant_of(k);
        const auto& rows = L.lg_rows[v];
        double* ls = lgrad_lam_stage(*s);
        for (size_t q = 0; q < rows.size(); ++q) {
            const long r = rows[q].first + long(rows[q].second) * k;
            if (r < 0 || r >= L.m) { ++bad_rows; continue; }   // (the device would read outside lambda)
            ls[q] = lambda[r];
        }
        const std::vector<LgradEntry>& ent = L.lg_ent[v];
        auto lam = [&](int e) { return ls[ent[size_t(e)].lam]; };
        auto jac = [&](int e) { return s->jac[ent[size_t(e)].slot]; };
        for (int c = 0; c < NXK; ++c)
            store(long(NXK) * k + c, lgrad_column(sigma, s->grad[c], L.lg_cbeg[v][size_t(c)], L.lg_cbeg[v][size_t(c) + 1], lam, jac));
        if (k == N - 1) {   // the horizon-global columns: no cost on them
            auto glam = [&](int e) { return ls[L.lg_glob[size_t(e)].lam]; };
            auto gjac = [&](int e) { return s->jac[L.lg_glob[size_t(e)].slot]; };
            for (int c = 0; c < NXG; ++c) store(long(NXK) * N + c, lgrad_column(sigma, 0.0, L.lg_gcbeg[size_t(c)], L.lg_gcbeg[size_t(c) + 1], glam, gjac));
        }
    }
    delete s;
    return bad_rows;
}

}  // extern "C"
