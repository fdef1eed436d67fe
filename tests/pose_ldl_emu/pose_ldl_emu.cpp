// TEST-ONLY CPU emulation of the pose finder's dense L D L^T kernels (hipnlp_pose.hip hipnlp_pose_saddle_ldl_kernel,
// hipnlp_pose_saddle_ldl_solve_kernel): the element expressions, the searches' join and the choice of the pivot are those of pose_ldl.h — the
// header the device compiles — but the elements are walked in ANOTHER order than the device's mapping: searches from the last index
// down, multipliers from the last row up, the trailing update row by row, the interchange as whole symmetric rows and columns, the
// forward solve row by row, the backward solve element by element.  Every element has one chain (pose_ldl.h), so the bits agree.
// The places of the stored entries are stated here from the vectors of PoseLayout, not from PoseLayout::fill_ldl_tables.
// It is NOT part of the product: libhipnlp.so does not contain it.
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../hippopt_amd/csrc/pose_layout.h"
#include "../../hippopt_amd/csrc/pose_ldl.h"

using namespace hipnlp;

namespace {

struct Handle {
    PoseLayout L;
    KinTables kt;
    PoseLdlTables tables;   // the device table, for the table test only
};

struct Factored {
    int status = PL_OK, pos = 0, neg = 0, zero = 0;
    int det_not_negative = 0;   // 2x2 blocks whose determinant is not negative (the emulation's assertion: stays 0)
};

// (i, j) of the symmetric matrix, either way round
double& sym(double* a, int N, int i, int j) { return i >= j ? a[pl_at(N, i, j)] : a[pl_at(N, j, i)]; }

Factored factor(int N, double* a, int* ipiv, int* perm, int* kind) {
    Factored f;
    std::vector<double> x0(size_t(N), 0.0), x1(size_t(N), 0.0);
    for (int i = 0; i < N; ++i) perm[i] = i;
    int k = 0;
    while (k < N) {
        const int kc = pl_col(N, k);
        const double akk = a[kc];
        PlMax cm = pl_max_none();
        for (int i = N - 1; i > k; --i) cm = pl_max_join(pl_max_of(a[kc + i - k], i), cm);
        bool bad = cm.bad || !minres_finite(akk);
        const double absakk = pl_abs(akk), colmax = cm.v < 0.0 ? 0.0 : cm.v;
        int kp = k, kstep = 1;
        double arr = 0.0;
        bool zero_column = false;
        if (!bad) {
            if (pl_column_is_zero(absakk, colmax)) zero_column = true;
            else if (!pl_keep_diagonal(absakk, colmax)) {
                const int imax = cm.at;
                PlMax rm = pl_max_none();
                for (int t = N - 1; t >= k; --t) if (t != imax) rm = pl_max_join(pl_max_of(sym(a, N, imax, t), t), rm);
                arr = a[pl_col(N, imax)];
                bad = rm.bad || !minres_finite(arr);
                if (!bad) { const PlPivot pv = pl_choose(k, imax, absakk, colmax, rm.v, pl_abs(arr)); kp = pv.kp; kstep = pv.kstep; }
            }
        }
        if (bad || zero_column) {
            for (int i = k; i < N; ++i) { ipiv[i] = i + 1; kind[i] = PL_ONE; }
            f.status = bad ? PL_NONFINITE : PL_SINGULAR;
            if (!bad) f.zero = 1;
            return f;
        }
        const int kk = k + kstep - 1, base = k + kstep;
        if (kp != kk) {
            for (int t = N - 1; t >= 0; --t) if (t != kk && t != kp) std::swap(sym(a, N, kk, t), sym(a, N, kp, t));
            std::swap(a[pl_col(N, kk)], a[pl_col(N, kp)]);
            std::swap(perm[kk], perm[kp]);
        }
        if (kstep == 1) {
            const double d = a[kc];
            if (d > 0.0) ++f.pos; else ++f.neg;
            ipiv[k] = kp + 1; kind[k] = PL_ONE;
            for (int i = N - 1; i >= base; --i) { x0[size_t(i)] = a[kc + i - k]; a[kc + i - k] = pl_l1(x0[size_t(i)], d); }
            for (int i = base; i < N; ++i)
                for (int j = base; j <= i; ++j) a[pl_at(N, i, j)] = pl_update1(a[pl_at(N, i, j)], x0[size_t(i)], a[kc + j - k]);
        } else {
            ++f.pos; ++f.neg;
            ipiv[k] = ipiv[k + 1] = -(kp + 1); kind[k] = PL_FIRST; kind[k + 1] = PL_SECOND;
            const int kc1 = pl_col(N, k + 1);
            const PlBlock blk = pl_block(a[kc], a[kc + 1], a[kc1]);
            if (!pl_block_det_negative(blk)) ++f.det_not_negative;
            for (int i = N - 1; i >= base; --i) {
                x0[size_t(i)] = a[kc + i - k]; x1[size_t(i)] = a[kc1 + i - k - 1];
                a[kc + i - k] = pl_w_first(blk, x0[size_t(i)], x1[size_t(i)]);
                a[kc1 + i - k - 1] = pl_w_second(blk, x0[size_t(i)], x1[size_t(i)]);
            }
            for (int i = base; i < N; ++i)
                for (int j = base; j <= i; ++j)
                    a[pl_at(N, i, j)] = pl_update2(a[pl_at(N, i, j)], x0[size_t(i)], x1[size_t(i)], a[kc + j - k], a[kc1 + j - k - 1]);
        }
        k = base;
    }
    return f;
}

// perm and kind from a stored pivot vector (a word that names no index of the trailing matrix interchanges nothing)
void scan(int N, const int* ipiv, int* perm, int* kind) {
    for (int i = 0; i < N; ++i) { perm[i] = i; kind[i] = PL_ONE; }
    int k = 0;
    while (k < N) {
        const int p = ipiv[k];
        const bool two = p < 0 && k + 1 < N;
        const int kk = two ? k + 1 : k;
        int kp = (p < 0 ? -p : p) - 1;
        if (kp < kk || kp >= N) kp = kk;
        if (two) { kind[k] = PL_FIRST; kind[k + 1] = PL_SECOND; }
        std::swap(perm[kk], perm[kp]);
        k = kk + 1;
    }
}

// b, x [N] in the order of K; every store to x counted
void solve(int N, const double* a, const int* perm, const int* kind, bool good, const double* b, double* x, int* writes) {
    std::vector<double> y(size_t(N), 0.0), z(size_t(N), 0.0);
    if (good) {
        for (int i = 0; i < N; ++i) y[size_t(i)] = b[perm[i]];
        for (int i = 0; i < N; ++i)
            for (int k = 0; k < i; ++k)
                if (!(i == k + 1 && kind[k] == PL_FIRST)) y[size_t(i)] = pl_axpy(y[size_t(i)], a[pl_at(N, i, k)], y[size_t(k)]);
        for (int i = N - 1; i >= 0; --i) {
            if (kind[i] == PL_ONE) z[size_t(i)] = pl_diag1(y[size_t(i)], a[pl_col(N, i)]);
            else if (kind[i] == PL_FIRST) z[size_t(i)] = pl_diag2_first(pl_solve_block(a[pl_col(N, i)], a[pl_col(N, i) + 1], a[pl_col(N, i + 1)]), y[size_t(i)], y[size_t(i) + 1]);
            else z[size_t(i)] = pl_diag2_second(pl_solve_block(a[pl_col(N, i - 1)], a[pl_col(N, i - 1) + 1], a[pl_col(N, i)]), y[size_t(i) - 1], y[size_t(i)]);
        }
        for (int k = N - 1; k >= 0; --k)
            for (int i = N - 1; i > k; --i)
                if (!(k == i - 1 && kind[i] == PL_SECOND)) z[size_t(k)] = pl_axpy(z[size_t(k)], a[pl_at(N, i, k)], z[size_t(i)]);
    }
    for (int i = N - 1; i >= 0; --i) { x[perm[i]] = good ? z[size_t(i)] : pl_nan(); writes[perm[i]]++; }
}

}  // namespace

extern "C" {

Handle* plemu_create(const hipnlp_pose_desc* desc, char* err, int errlen) {
    Handle* h = new Handle();
    std::string e;
    if (Layout::make_kin_tables(desc->model, h->kt, e)) Layout::fill_terrain_tops(h->kt, desc->settings.terrain, desc->settings.n_terrain_steps, desc->settings.terrain_steps);
    if (e.empty() && !h->L.build(desc->settings, h->kt)) e = h->L.error;
    if (e.empty() && !h->L.ldl_fits()) e = h->L.error;
    if (!e.empty()) {
        std::strncpy(err, e.c_str(), size_t(errlen - 1));
        delete h;
        return nullptr;
    }
    h->L.fill_ldl_tables(h->tables);
    return h;
}
void plemu_destroy(Handle* h) { delete h; }
void plemu_dims(const Handle* h, int* n, int* m, int* nnz, int* hnnz) { *n = h->L.n; *m = h->L.m; *nnz = h->L.nnz; *hnnz = h->L.hnnz; }
void plemu_sparsity(const Handle* h, int* irow, int* jcol, int* hrow, int* hcol) {
    for (int i = 0; i < h->L.nnz; ++i) { irow[i] = h->L.irow[size_t(i)]; jcol[i] = h->L.jcol[size_t(i)]; }
    for (int i = 0; i < h->L.hnnz; ++i) { hrow[i] = h->L.hrow[size_t(i)]; hcol[i] = h->L.hcol[size_t(i)]; }
}
// [0] the largest order, [1] its packed doubles, [2] right-hand sides, [3] tries, [4] entries of the Hessian staged, [5] entries of jac g staged
void plemu_caps(int* out) { out[0] = PL_MAX_N; out[1] = PL_MAX_DOUBLES; out[2] = PL_MAX_NRHS; out[3] = PL_MAX_TRIES; out[4] = PK_HESS_CAP; out[5] = PP_ENT_CAP; }
// the device table (PoseLayout::fill_ldl_tables): hess_at [PK_HESS_CAP], jac_at [PP_ENT_CAP]
void plemu_device_words(const Handle* h, int* hess_at, int* jac_at) {
    std::memcpy(hess_at, h->tables.hess_at, sizeof(h->tables.hess_at));
    std::memcpy(jac_at, h->tables.jac_at, sizeof(h->tables.jac_at));
}
// whether PoseLayout::ldl_fits would refuse a pattern of m rows (the order alone)
int plemu_order_fits(int m) { return POSE_NX + m <= PL_MAX_N; }

// ---- the factorisation and the solve at a general order (packed lower triangle, column major) ----------------------------------------------
// a [N (N + 1) / 2] in place; ipiv, perm, kind [N]; out [5]: status, positive, negative, zero, 2x2 blocks whose determinant is not negative
void plemu_factor_general(int N, double* a, int* ipiv, int* perm, int* kind, int* out) {
    const Factored f = factor(N, a, ipiv, perm, kind);
    out[0] = f.status; out[1] = f.pos; out[2] = f.neg; out[3] = f.zero; out[4] = f.det_not_negative;
}
void plemu_solve_general(int N, const double* a, const int* ipiv, const double* b, double* x, int* writes) {
    std::vector<int> perm(size_t(N), 0), kind(size_t(N), 0);
    scan(N, ipiv, perm.data(), kind.data());
    solve(N, a, perm.data(), kind.data(), true, b, x, writes);
}

// ---- hipnlp_pose_saddle_ldl_kernel, one pose -----------------------------------------------------------------------------------------------
// rhs / sol [nrhs][81], [nrhs][m]; inertia [3]; scalars [2]: status, tries; delta [1]; factor [N (N + 1) / 2] and pivots [N] or both null;
// writes_top / writes_bottom count the stores to the solutions; returns the 2x2 blocks whose determinant is not negative, over all tries
int plemu_factor(const Handle* h, const double* hess, const double* jac, const double* dx, const double* dc, int nrhs, const double* rhs_top, const double* rhs_bottom,
                 double* sol_top, int* writes_top, double* sol_bottom, int* writes_bottom, int* inertia, int* scalars, double* delta_out, double delta_init, double kappa,
                 int max_tries, double* factor_out, int* pivots_out) {
    const PoseLayout& L = h->L;
    const int m = L.m, N = POSE_NX + m, nd = pl_doubles(N);
    std::vector<double> a(size_t(nd), 0.0);
    std::vector<int> ipiv(size_t(N), 0), perm(size_t(N), 0), kind(size_t(N), 0);
    double delta = 0.0;
    int t = 0, status = PL_OK, det_bad = 0;
    Factored f;
    for (;;) {
        for (int e = nd - 1; e >= 0; --e) a[size_t(e)] = 0.0;
        for (int e = L.nnz - 1; e >= 0; --e) a[size_t(pl_at(N, POSE_NX + L.irow[size_t(e)], L.jcol[size_t(e)]))] = jac[e];
        for (int e = L.hnnz - 1; e >= 0; --e) a[size_t(pl_at(N, L.hrow[size_t(e)], L.hcol[size_t(e)]))] = hess[e];
        for (int i = m - 1; i >= 0; --i) a[size_t(pl_col(N, POSE_NX + i))] = pl_diag_bottom(dc != nullptr, dc ? dc[i] : 0.0);
        for (int c = POSE_NX - 1; c >= 0; --c) a[size_t(pl_col(N, c))] = pl_diag_top(a[size_t(pl_col(N, c))], dx != nullptr, dx ? dx[c] : 0.0, t > 0, delta);
        f = factor(N, a.data(), ipiv.data(), perm.data(), kind.data());
        det_bad += f.det_not_negative;
        const bool wanted = pl_inertia_wanted(f.pos, f.neg, f.zero, m);
        status = pl_final_status(f.status, wanted, max_tries);
        if (!pl_ladder_goes_on(f.status, wanted, t, max_tries)) break;
        ++t;
        delta = pl_next_delta(t, delta, delta_init, kappa);
    }
    inertia[0] = f.pos; inertia[1] = f.neg; inertia[2] = f.zero;
    scalars[0] = status; scalars[1] = t;
    *delta_out = delta;
    if (factor_out) { std::memcpy(factor_out, a.data(), sizeof(double) * size_t(nd)); for (int i = 0; i < N; ++i) pivots_out[i] = ipiv[size_t(i)]; }
    std::vector<double> b(size_t(N), 0.0), x(size_t(N), 0.0);
    std::vector<int> w(size_t(N), 0);
    for (int r = 0; r < nrhs; ++r) {
        for (int i = 0; i < POSE_NX; ++i) b[size_t(i)] = rhs_top[r * POSE_NX + i];
        for (int i = 0; i < m; ++i) b[size_t(POSE_NX + i)] = rhs_bottom[r * m + i];
        std::fill(w.begin(), w.end(), 0);
        solve(N, a.data(), perm.data(), kind.data(), status == PL_OK || status == PL_EXHAUSTED, b.data(), x.data(), w.data());
        for (int i = 0; i < POSE_NX; ++i) { sol_top[r * POSE_NX + i] = x[size_t(i)]; writes_top[r * POSE_NX + i] += w[size_t(i)]; }
        for (int i = 0; i < m; ++i) { sol_bottom[r * m + i] = x[size_t(POSE_NX + i)]; writes_bottom[r * m + i] += w[size_t(POSE_NX + i)]; }
    }
    return det_bad;
}

// ---- hipnlp_pose_saddle_ldl_solve_kernel, one pose -----------------------------------------------------------------------------------------
void plemu_solve(const Handle* h, const double* factor_in, const int* pivots, int nrhs, const double* rhs_top, const double* rhs_bottom, double* sol_top, double* sol_bottom) {
    const int m = h->L.m, N = POSE_NX + m;
    std::vector<double> b(size_t(N), 0.0), x(size_t(N), 0.0);
    std::vector<int> w(size_t(N), 0);
    for (int r = 0; r < nrhs; ++r) {
        for (int i = 0; i < POSE_NX; ++i) b[size_t(i)] = rhs_top[r * POSE_NX + i];
        for (int i = 0; i < m; ++i) b[size_t(POSE_NX + i)] = rhs_bottom[r * m + i];
        plemu_solve_general(N, factor_in, pivots, b.data(), x.data(), w.data());
        for (int i = 0; i < POSE_NX; ++i) sol_top[r * POSE_NX + i] = x[size_t(i)];
        for (int i = 0; i < m; ++i) sol_bottom[r * m + i] = x[size_t(POSE_NX + i)];
    }
}

// ---- what the entry points refuse (pose_ldl.h): 1 and the reason in msg, or 0 ---------------------------------------------------------------
int plemu_factor_call_error(int hess, int jac, int nrhs, int rhs_top, int rhs_bottom, int sol_top, int sol_bottom, int inertia, int status, double delta_init, double kappa,
                            int max_tries, int factor_ptr, int pivots, char* msg, int msglen) {
    const char* e = pl_factor_call_error(hess, jac, nrhs, rhs_top, rhs_bottom, sol_top, sol_bottom, inertia, status, delta_init, kappa, max_tries, factor_ptr, pivots);
    if (e) std::strncpy(msg, e, size_t(msglen - 1));
    return e != nullptr;
}
int plemu_solve_call_error(int factor_ptr, int pivots, int nrhs, int rhs_top, int rhs_bottom, int sol_top, int sol_bottom, char* msg, int msglen) {
    const char* e = pl_solve_call_error(factor_ptr, pivots, nrhs, rhs_top, rhs_bottom, sol_top, sol_bottom);
    if (e) std::strncpy(msg, e, size_t(msglen - 1));
    return e != nullptr;
}

}  // extern "C"
