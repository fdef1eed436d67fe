// TEST-ONLY CPU emulation of the condensed block factorisation of the KKT solve (hipnlp.hip hipnlp_kkt_condensed_factor_kernel): the
// expressions — s = 1 / d_c, the term of an element, the reciprocal of the diagonal — are knot_condense.h's, the header the device compiles,
// but the pairs of an element are NOT found through KnotCondenseTables: the knot's column block is read from the pattern vectors
// irow / jcol of Layout, every column's entries are sorted by global row here, and the elements are walked from the last one down.  Every
// element has one chain in ascending global row (knot_condense.h), so the bits agree.  The factorisation is tests/kkt_block_emu's, in
// its own element order.  The block preconditioner's, the diagonal's, the solve's and the operator's emulations are compiled into this
// library as they stand, so that all of them share one handle.  It is NOT part of the product: libhipnlp.so does not contain it.
#include "../kkt_block_emu/kkt_block_emu.cpp"

#include "../../hippopt_amd/csrc/knot_condense.h"

namespace {

struct ColEntry { long row; double val; };

// the column block of knot k from the pattern: [189] lists in ascending global row
std::vector<std::vector<ColEntry>> column_block(const Layout& L, const double* jac, int k) {
    std::vector<std::vector<ColEntry>> cols;
    cols.resize(NXK);
    const long base = L.jac_base(k);
    const int len = L.nnz_v[L.variant_of(k)];
    for (int p = len - 1; p >= 0; --p) {
        const int c = L.jcol[size_t(base + p)] - NXK * k;
        cols[size_t(c)].push_back({long(L.irow[size_t(base + p)]), jac[base + p]});
    }
    for (auto& c : cols) std::sort(c.begin(), c.end(), [](const ColEntry& a, const ColEntry& b) { return a.row < b.row; });
    return cols;
}

// B_k into the packed triangle a; returns whether every d_c of a row touching the block is a finite number > 0; terms [KL_DOUBLES] or
// null: the number of fused multiply-adds of every element
bool condensed_assemble(const kktemu_handle* h, int k, const double* hess, const double* jac, const double* dx, const double* dc, double* a, int* terms) {
    constexpr int N = KL_N;
    const HessLayout& HL = h->HL;
    const double* hk = hess + HL.knot_base(k);
    const double* dxk = dx ? dx + size_t(NXK) * k : nullptr;
    for (int q = KL_DOUBLES - 1; q >= 0; --q) a[q] = 0.0;
    for (int p = HL.nnz_knot - 1; p >= 0; --p) a[pl_at(N, HL.lrow[size_t(p)], HL.lcol[size_t(p)])] = hk[p];
    for (int c = N - 1; c >= 0; --c) a[pl_col(N, c)] = pl_diag_top(a[pl_col(N, c)], dxk != nullptr, dxk ? dxk[c] : 0.0, false, 0.0);
    const std::vector<std::vector<ColEntry>> cols = column_block(h->L, jac, k);
    bool good = true;
    for (const auto& c : cols) for (const ColEntry& e : c) good = good && kc_scale_good(kc_scale(dc[e.row]));
    for (int r = N - 1; r >= 0; --r)
        for (int c = r; c >= 0; --c) {
            double acc = a[pl_at(N, r, c)];
            int count = 0;
            for (const ColEntry& ec : cols[size_t(c)])        // ascending global row
                for (const ColEntry& er : cols[size_t(r)])
                    if (er.row == ec.row) { acc = kc_term(acc, er.val, ec.val, kc_scale(dc[ec.row])); ++count; }
            a[pl_at(N, r, c)] = acc;
            if (terms) terms[pl_at(N, r, c)] = count;
        }
    return good;
}

}  // namespace

extern "C" {

// [0] KC_ENT_MAX, [1] KC_ROW_MAX, [2] whether the layout's tables can be built (kc_build_tables), [3] entries of the largest column block,
// [4] rows touching the block that most rows touch
void kcemu_caps(const kktemu_handle* h, int* out) {
    KnotCondenseTables* t = new KnotCondenseTables();
    std::string err;
    out[0] = KC_ENT_MAX; out[1] = KC_ROW_MAX;
    out[2] = kc_build_tables(h->L, *t, err) ? 1 : 0;
    out[3] = std::max(t->nent[0], std::max(t->nent[1], t->nent[2]));
    out[4] = std::max(t->nrows[0], std::max(t->nrows[1], t->nrows[2]));
    delete t;
}

// the assembled B_k of knot k [KL_DOUBLES] and the number of terms of every element; returns 1 where every d_c touching the block is good
int kcemu_assemble(const kktemu_handle* h, int k, const double* hess, const double* jac, const double* dx, const double* dc, double* a, int* terms) {
    return condensed_assemble(h, k, hess, jac, dx, dc, a, terms) ? 1 : 0;
}

// the same block through the DEVICE tables (kc_build_tables) and the device's merge (kc_element), staged as the kernel stages them; also
// the six globals' accumulated diagonal [NXG] as the last knot's threads sum it.  Returns 0 where the tables cannot be built, and -1 where
// a table word points outside what the kernel stages (the kernel clamps; the tables must not need it)
int kcemu_assemble_tables(const kktemu_handle* h, int k, const double* hess, const double* jac, const double* dx, const double* dc, double* a, double* glob) {
    constexpr int N = KL_N;
    const Layout& L = h->L;
    const HessLayout& HL = h->HL;
    KnotCondenseTables* t = new KnotCondenseTables();
    std::string err;
    if (!kc_build_tables(L, *t, err)) { delete t; return 0; }
    const int v = L.variant_of(k), ne = t->nent[v], nr = t->nrows[v], blen = L.nnz_v[v];
    const double* jv = jac + L.jac_base(k);
    std::vector<double> sv(KC_ENT_CAP, 0.0), ss(KC_ROW_CAP, 0.0);
    int rc = 1;
    if (ne > KC_ENT_CAP || nr > KC_ROW_CAP) rc = -1;
    for (int e = 0; e < ne && rc == 1; ++e) {
        if (t->pos[v][e] >= blen || t->rank[v][e] >= nr) { rc = -1; break; }
        sv[size_t(e)] = jv[t->pos[v][e]];
    }
    for (int q = 0; q < nr && rc == 1; ++q) {
        const long r = long(t->row_a[v][q]) + long(t->row_b[v][q]) * k;
        if (r < 0 || r >= L.m) { rc = -1; break; }
        ss[size_t(q)] = kc_scale(dc[r]);
    }
    for (int c = 0; c <= N && rc == 1; ++c) if (t->cbeg[v][c] > ne || (c > 0 && t->cbeg[v][c - 1] > t->cbeg[v][c])) rc = -1;
    if (rc == 1) {
        const double* hk = hess + HL.knot_base(k);
        const double* dxk = dx ? dx + size_t(NXK) * k : nullptr;
        for (int q = 0; q < KL_DOUBLES; ++q) a[q] = 0.0;
        for (int p = 0; p < HL.nnz_knot; ++p) a[pl_at(N, HL.lrow[size_t(p)], HL.lcol[size_t(p)])] = hk[p];
        for (int c = 0; c < N; ++c) a[pl_col(N, c)] = pl_diag_top(a[pl_col(N, c)], dxk != nullptr, dxk ? dxk[c] : 0.0, false, 0.0);
        for (int j = 0; j < N; ++j)
            for (int i = j; i < N; ++i)
                a[pl_at(N, i, j)] = kc_element(a[pl_at(N, i, j)], int(t->cbeg[v][i]), int(t->cbeg[v][i + 1]), int(t->cbeg[v][j]), int(t->cbeg[v][j + 1]),
                                               [&](int e) { return int(t->rank[v][e]); }, [&](int e) { return sv[size_t(e)]; }, [&](int q) { return ss[size_t(q)]; });
        for (int g = 0; g < NXG; ++g) {
            double acc = dx ? dx[size_t(NXK) * L.N + g] : 0.0;
            for (int e = t->gbeg[g]; e < t->gbeg[g + 1]; ++e) {
                if (e >= JP_GLOB_CAP || t->gpos[e] < 0 || t->gpos[e] >= int(L.jperm_glob.size()) || t->grow[e] < 0 || t->grow[e] >= L.m) { rc = -1; break; }
                const double aj = jac[L.jac_glob_base + t->gpos[e]];
                acc = kc_term(acc, aj, aj, kc_scale(dc[t->grow[e]]));
            }
            glob[g] = acc;
        }
    }
    delete t;
    return rc;
}

// hipnlp_kkt_condensed_factor_kernel, one trajectory: kbemu_factor's arrays plus minv_top [n], minv_bottom [m] and the stores counted
void kcemu_factor(const kktemu_handle* h, const double* hess, const double* jac, const double* dx, const double* dc, double floor, double* factor, int* words, double* e, double* o,
                  int* inertia, int* status, double* minv_top, double* minv_bottom, int* top_writes, int* bottom_writes, int* checks) {
    constexpr int NB = KL_N;
    const Layout& L = h->L;
    const int N = L.N;
    checks[0] = checks[1] = 0;
    for (int k = N - 1; k >= 0; --k) {   // (the knots are independent: any order)
        double* a = factor + size_t(k) * KL_DOUBLES;
        int* w = words + size_t(k) * NB;
        double* ek = e + size_t(k) * NB;
        double* ok = o + size_t(k) * NB;
        const bool dc_good = condensed_assemble(h, k, hess, jac, dx, dc, a, nullptr);
        for (int c = 0; c < NB; ++c) { minv_top[size_t(NXK) * k + c] = kc_top(a[pl_col(NB, c)], floor); top_writes[size_t(NXK) * k + c]++; }
        std::vector<int> ipiv(size_t(NB), 0), perm(size_t(NB), 0), kind(size_t(NB), 0);
        BlockFactored f;
        if (dc_good) f = block_factor(a, ipiv.data(), perm.data(), kind.data());
        else f.status = KL_NONFINITE;
        if (f.status != KL_OK) {
            for (int q = 0; q < KL_DOUBLES; ++q) a[q] = pl_nan();
            for (int i = 0; i < NB; ++i) { w[i] = kl_word(i + 1, i, PL_ONE); ek[i] = ok[i] = pl_nan(); }
            f.pos = f.neg = f.zero = 0;
        } else {
            for (int i = NB - 1; i >= 0; --i) {
                w[i] = kl_word(ipiv[size_t(i)], perm[size_t(i)], kind[size_t(i)]);
                ok[i] = 0.0;
                if (kind[size_t(i)] == PL_ONE) ek[i] = kl_floored_inverse(a[pl_col(NB, i)], floor);
                else if (kind[size_t(i)] == PL_FIRST) {
                    const KlAbsInv2 q = kl_abs_inverse2(a[pl_col(NB, i)], a[pl_col(NB, i) + 1], a[pl_col(NB, i + 1)], floor);
                    ek[i] = q.e0; ok[i] = q.o;
                    if (!kl_block_positive_definite(q.e0, q.e1, q.o)) ++checks[1];
                } else ek[i] = kl_abs_inverse2(a[pl_col(NB, i - 1)], a[pl_col(NB, i - 1) + 1], a[pl_col(NB, i)], floor).e1;
            }
            checks[0] += f.det_not_negative;
        }
        inertia[3 * k + 0] = f.pos; inertia[3 * k + 1] = f.neg; inertia[3 * k + 2] = f.zero;
        status[k] = f.status;
        // the bottom: the rows minres_owned gives the knot
        const int pv = L.pair_variant_of(k);
        for (int q = JP_ROW_CAP - 1; q >= 0; --q) {
            const int32_t ra = h->T.row_a[pv][q];
            if (ra == G_NONE) continue;
            const long i = ra + long(h->T.row_b[pv][q]) * k;
            minv_bottom[i] = kc_scale(dc[i]);
            bottom_writes[i]++;
        }
    }
    // the six globals, from the pattern: the entries of every global column in ascending row
    for (int g = 0; g < NXG; ++g) {
        std::vector<ColEntry> col;
        for (long p = L.jac_glob_base; p < L.nnz; ++p)
            if (L.jcol[size_t(p)] == NXK * N + g) col.push_back({long(L.irow[size_t(p)]), jac[p]});
        std::sort(col.begin(), col.end(), [](const ColEntry& a, const ColEntry& b) { return a.row < b.row; });
        double acc = dx ? dx[size_t(NXK) * N + g] : 0.0;
        for (const ColEntry& c : col) acc = kc_term(acc, c.val, c.val, kc_scale(dc[c.row]));
        minv_top[size_t(NXK) * N + g] = kc_top(acc, floor);
        top_writes[size_t(NXK) * N + g]++;
    }
}

// what the entry point refuses (knot_condense.h): 1 and the reason in msg, or 0
int kcemu_factor_call_error(int hess, int jac, int dc, double floor, int factor, int pivots, int e, int o, int inertia, int status, int minv_top, int minv_bottom, char* msg,
                            int msglen) {
    const char* r = kc_factor_call_error(hess, jac, dc, floor, factor, pivots, e, o, inertia, status, minv_top, minv_bottom);
    if (r) std::strncpy(msg, r, size_t(msglen - 1));
    return r != nullptr;
}

}  // extern "C"
