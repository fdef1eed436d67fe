// TEST-ONLY CPU emulation of the block preconditioner of the KKT solve (hipnlp.hip hipnlp_kkt_block_factor_kernel,
// hipnlp_kkt_block_apply_kernel, hipnlp_kkt_minres_block_first_kernel): the element expressions, the searches' join, the choice of the
// pivot, |D|^-1 and the three-term diagonal are those of knot_ldl.h and pose_ldl.h — the headers the device compiles — but the elements
// are walked in ANOTHER order than the device's mapping: searches from the last index down, multipliers from the last row up, the trailing
// update row by row, the interchange as whole symmetric rows and columns, the forward solve row by row, the backward solve element by
// element.  Every element has one chain (knot_ldl.h), so the bits agree.  The places of the stored entries are stated here from the
// vectors of HessLayout, not from HessLayout::fill_ldl_tables.  The diagonal's, the solve's and the operator's emulations are compiled into
// this library as they stand, so that all of them share one handle.  It is NOT part of the product: libhipnlp.so does not contain it.
#include "../kkt_precond_emu/kkt_precond_emu.cpp"

#include "../../hippopt_amd/csrc/knot_ldl.h"

namespace {

struct BlockFactored {
    int status = KL_OK, pos = 0, neg = 0, zero = 0;
    int det_not_negative = 0;   // 2x2 blocks whose determinant is not negative (stays 0)
};

double& bsym(double* a, int N, int i, int j) { return i >= j ? a[pl_at(N, i, j)] : a[pl_at(N, j, i)]; }

BlockFactored block_factor(double* a, int* ipiv, int* perm, int* kind) {
    constexpr int N = KL_N;
    BlockFactored f;
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
                for (int t = N - 1; t >= k; --t) if (t != imax) rm = pl_max_join(pl_max_of(bsym(a, N, imax, t), t), rm);
                arr = a[pl_col(N, imax)];
                bad = rm.bad || !minres_finite(arr);
                if (!bad) { const PlPivot pv = pl_choose(k, imax, absakk, colmax, rm.v, pl_abs(arr)); kp = pv.kp; kstep = pv.kstep; }
            }
        }
        if (bad) { f.status = KL_NONFINITE; return f; }
        if (zero_column) {   // the step of a 1x1 pivot that moves nothing
            ++f.zero;
            ipiv[k] = k + 1; kind[k] = PL_ONE;
            k = k + 1;
            continue;
        }
        const int kk = k + kstep - 1, base = k + kstep;
        if (kp != kk) {
            for (int t = N - 1; t >= 0; --t) if (t != kk && t != kp) std::swap(bsym(a, N, kk, t), bsym(a, N, kp, t));
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

// one knot's record: hess the knot's block of the run; dx the knot's 189 elements or null.  Returns BlockFactored; *not_pd counts the 2x2
// blocks of |D|^-1 that are not positive definite (the emulation's assertion: stays 0)
BlockFactored block_record(const HessLayout& HL, const double* hess, const double* dx, double floor, double* factor, int* words, double* e, double* o, int* not_pd) {
    constexpr int N = KL_N;
    std::vector<int> ipiv(size_t(N), 0), perm(size_t(N), 0), kind(size_t(N), 0);
    for (int q = KL_DOUBLES - 1; q >= 0; --q) factor[q] = 0.0;
    for (int p = HL.nnz_knot - 1; p >= 0; --p) factor[pl_at(N, HL.lrow[size_t(p)], HL.lcol[size_t(p)])] = hess[p];
    for (int c = N - 1; c >= 0; --c) factor[pl_col(N, c)] = pl_diag_top(factor[pl_col(N, c)], dx != nullptr, dx ? dx[c] : 0.0, false, 0.0);
    BlockFactored f = block_factor(factor, ipiv.data(), perm.data(), kind.data());
    if (f.status != KL_OK) {
        for (int q = 0; q < KL_DOUBLES; ++q) factor[q] = pl_nan();
        for (int i = 0; i < N; ++i) { words[i] = kl_word(i + 1, i, PL_ONE); e[i] = o[i] = pl_nan(); }
        f.pos = f.neg = f.zero = 0;
        return f;
    }
    for (int i = N - 1; i >= 0; --i) {
        words[i] = kl_word(ipiv[size_t(i)], perm[size_t(i)], kind[size_t(i)]);
        o[i] = 0.0;
        if (kind[size_t(i)] == PL_ONE) e[i] = kl_floored_inverse(factor[pl_col(N, i)], floor);
        else if (kind[size_t(i)] == PL_FIRST) {
            const KlAbsInv2 q = kl_abs_inverse2(factor[pl_col(N, i)], factor[pl_col(N, i) + 1], factor[pl_col(N, i + 1)], floor);
            e[i] = q.e0; o[i] = q.o;
            if (!kl_block_positive_definite(q.e0, q.e1, q.o)) ++*not_pd;
        } else e[i] = kl_abs_inverse2(factor[pl_col(N, i - 1)], factor[pl_col(N, i - 1) + 1], factor[pl_col(N, i)], floor).e1;
    }
    return f;
}

// z [189] = P^T L^-T |D|^-1 L^-1 P r of one knot from its record; every store to z counted
void block_apply(const double* a, const int* words, const double* e, const double* o, const double* r, double* z, int* writes) {
    constexpr int N = KL_N;
    std::vector<double> y(size_t(N), 0.0), t(size_t(N), 0.0);
    const bool good = kl_good(e[0]);
    auto put = [&](int i, double v) { const int p = kl_word_perm(words[i]); if (p < N) { z[p] = v; if (writes) writes[p]++; } };
    if (!good) {
        for (int i = N - 1; i >= 0; --i) put(i, pl_nan());
        return;
    }
    auto first = [&](int i) { return kl_word_kind(words[i]) == PL_FIRST; };
    for (int i = 0; i < N; ++i) { const int p = kl_word_perm(words[i]); y[size_t(i)] = r[p < N ? p : 0]; }
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < i; ++k)
            if (!(i == k + 1 && first(k))) y[size_t(i)] = pl_axpy(y[size_t(i)], a[pl_at(N, i, k)], y[size_t(k)]);
    for (int i = N - 1; i >= 0; --i)
        t[size_t(i)] = kl_diag3(e[i], y[size_t(i)], o[i], i + 1 < N ? y[size_t(i) + 1] : 0.0, i > 0 ? o[i - 1] : 0.0, i > 0 ? y[size_t(i) - 1] : 0.0);
    for (int k = N - 1; k >= 0; --k)
        for (int i = N - 1; i > k; --i)
            if (!(k == i - 1 && first(k))) t[size_t(k)] = pl_axpy(t[size_t(k)], a[pl_at(N, i, k)], t[size_t(i)]);
    for (int i = N - 1; i >= 0; --i) put(i, t[size_t(i)]);
}

// the solve of tests/kkt_minres_emu with hipnlp_kkt_minres_block_first_kernel in the place of the first launch
struct BlockSolve : Solve {
    const double *factor, *be, *bo;
    const int* words;

    void first_block(int it) {
        const bool init = it == 0;
        double c2 = 0.0;
        if (!init) {
            const MinresRec& in = rec[(it - 1) & 1];
            if (in.status != MINRES_RUNNING) return;
            c2 = minres_div(minres_sum(part_a.data(), N), in.beta);
        }
        // the new r2 of an element, and what the launch stores beside y
        auto new_r2 = [&](int e, const double* rhs, std::vector<double> Vecs::*half, double* z, int* zw) {
            const size_t i = size_t(e);
            double r;
            if (init) {
                r = rhs[i];
                (vec[MR_W].*half)[i] = 0.0; (vec[MR_W2].*half)[i] = 0.0; z[i] = 0.0; zw[i]++;
                (vec[MR_R1].*half)[i] = r;
            } else {
                const double old = (vec[MR_R2].*half)[i];
                r = minres_new_r2(c2, old, (vec[MR_Y].*half)[i]);
                (vec[MR_R1].*half)[i] = old;
            }
            (vec[MR_R2].*half)[i] = r;
            return r;
        };
        for (int k = 0; k < N; ++k) {
            std::vector<double> rt(JP_WG, 0.0), rr0(JP_WG, 0.0), rr1(JP_WG, 0.0), r2s(KL_N, 0.0), ys(KL_N, 0.0);
            for (int tid = JP_WG - 1; tid >= 0; --tid) {
                const MinresOwned o = minres_owned(tid, k, N, row_a(k), row_b(k));
                if (o.top >= 0) rt[size_t(tid)] = new_r2(o.top, rhs_top, &Vecs::top, z_top, z_top_writes);
                if (o.row[0] >= 0) rr0[size_t(tid)] = new_r2(o.row[0], rhs_bottom, &Vecs::bottom, z_bottom, z_bottom_writes);
                if (o.row[1] >= 0) rr1[size_t(tid)] = new_r2(o.row[1], rhs_bottom, &Vecs::bottom, z_bottom, z_bottom_writes);
                if (tid < KL_N) r2s[size_t(tid)] = rt[size_t(tid)];
            }
            block_apply(factor + size_t(k) * KL_DOUBLES, words + size_t(k) * KL_N, be + size_t(k) * KL_N, bo + size_t(k) * KL_N, r2s.data(), ys.data(), nullptr);
            double prod[JP_WG];
            for (int tid = 0; tid < JP_WG; ++tid) {   // the thread's chain: top element, first row, second row
                const MinresOwned o = minres_owned(tid, k, N, row_a(k), row_b(k));
                double acc = 0.0;
                if (o.top >= 0) {
                    const double ym = tid < KL_N ? ys[size_t(tid)] : minres_precond(true, minv_top[o.top], rt[size_t(tid)]);
                    vec[MR_Y].top[size_t(o.top)] = ym;
                    acc = fm_fma(rt[size_t(tid)], ym, acc);
                }
                for (int q = 0; q < 2; ++q)
                    if (o.row[q] >= 0) {
                        const double r = q == 0 ? rr0[size_t(tid)] : rr1[size_t(tid)];
                        const double ym = minres_precond(true, minv_bottom[o.row[q]], r);
                        vec[MR_Y].bottom[size_t(o.row[q])] = ym;
                        acc = fm_fma(r, ym, acc);
                    }
                prod[tid] = acc;
            }
            part_b[size_t(k)] = jprod_dot_tree(prod);
        }
    }
};

}  // namespace

extern "C" {

// [0] the order of a block, [1] its packed doubles, [2] the entries the device table holds
void kbemu_caps(int* out) { out[0] = KL_N; out[1] = KL_DOUBLES; out[2] = KL_ENT_CAP; }
// the device table (HessLayout::fill_ldl_tables) [KL_ENT_CAP], and the block pattern lrow / lcol [nnz_knot]; returns nnz_knot
int kbemu_device_words(const kktemu_handle* h, int* at, int* lrow, int* lcol) {
    KnotLdlTables* t = new KnotLdlTables();
    h->HL.fill_ldl_tables(*t);
    std::memcpy(at, t->at, sizeof(t->at));
    delete t;
    for (int p = 0; p < h->HL.nnz_knot; ++p) { lrow[p] = h->HL.lrow[size_t(p)]; lcol[p] = h->HL.lcol[size_t(p)]; }
    return h->HL.nnz_knot;
}
int kbemu_nnz_knot(const kktemu_handle* h) { return h->HL.nnz_knot; }
int kbemu_fits(const kktemu_handle* h) { return h->HL.ldl_fits() ? 1 : 0; }

// hipnlp_kkt_block_factor_kernel, one trajectory: factor [N][KL_DOUBLES], words / e / o [N][189], inertia [N][3], status [N]; checks [2]:
// 2x2 pivot blocks whose determinant is not negative, 2x2 blocks of |D|^-1 that are not positive definite
void kbemu_factor(const kktemu_handle* h, const double* hess, const double* dx, double floor, double* factor, int* words, double* e, double* o, int* inertia, int* status,
                  int* checks) {
    const int N = h->L.N;
    checks[0] = checks[1] = 0;
    for (int k = 0; k < N; ++k) {
        const BlockFactored f = block_record(h->HL, hess + h->HL.knot_base(k), dx ? dx + size_t(NXK) * k : nullptr, floor, factor + size_t(k) * KL_DOUBLES, words + size_t(k) * KL_N,
                                             e + size_t(k) * KL_N, o + size_t(k) * KL_N, &checks[1]);
        inertia[3 * k + 0] = f.pos; inertia[3 * k + 1] = f.neg; inertia[3 * k + 2] = f.zero;
        status[k] = f.status;
        checks[0] += f.det_not_negative;
    }
}

// hipnlp_kkt_block_apply_kernel, one trajectory; the stores are counted
void kbemu_apply(const kktemu_handle* h, const double* factor, const int* words, const double* e, const double* o, const double* minv_top, const double* minv_bottom,
                 const double* r_top, const double* r_bottom, double* z_top, double* z_bottom, int* top_writes, int* bottom_writes) {
    const Layout& L = h->L;
    const int N = L.N;
    for (int k = 0; k < N; ++k) {
        block_apply(factor + size_t(k) * KL_DOUBLES, words + size_t(k) * KL_N, e + size_t(k) * KL_N, o + size_t(k) * KL_N, r_top + size_t(NXK) * k, z_top + size_t(NXK) * k,
                    top_writes + size_t(NXK) * k);
        const int pv = L.pair_variant_of(k);
        for (int q = JP_ROW_CAP - 1; q >= 0; --q) {
            const int32_t ra = h->T.row_a[pv][q];
            if (ra == G_NONE) continue;
            const long i = ra + long(h->T.row_b[pv][q]) * k;
            z_bottom[i] = minres_precond(true, minv_bottom[i], r_bottom[i]);
            bottom_writes[i]++;
        }
        if (k == N - 1)
            for (int c = 0; c < NXG; ++c) {
                const long i = long(NXK) * N + c;
                z_top[i] = minres_precond(true, minv_top[i], r_top[i]);
                top_writes[i]++;
            }
    }
}

// hipnlp_kkt_minres_block_device, one trajectory: kmremu_solve's arguments (without the traces) plus the stored record arrays
void kbemu_solve(const kktemu_handle* h, const double* hess, const double* jac, const double* dx, const double* dc, const double* factor, const int* words, const double* e,
                 const double* o, const double* minv_top, const double* minv_bottom, const double* rhs_top, const double* rhs_bottom, double* sol_top, double* sol_bottom,
                 double rtol, int maxit, int launched, int* iterations, double* residual, int* status, int* top_writes, int* bottom_writes, int* scalar_writes) {
    BlockSolve s;
    s.h = h; s.hess = hess; s.jac = jac; s.dx = dx; s.dc = dc; s.minv_top = minv_top; s.minv_bottom = minv_bottom; s.rhs_top = rhs_top; s.rhs_bottom = rhs_bottom;
    s.z_top = sol_top; s.z_bottom = sol_bottom; s.z_top_writes = top_writes; s.z_bottom_writes = bottom_writes; s.scalar_writes = scalar_writes;
    s.rtol = rtol; s.maxit = maxit; s.N = h->L.N; s.n = h->L.n; s.m = h->L.m;
    s.iterations = iterations; s.residual = residual; s.status = status;
    s.factor = factor; s.words = words; s.be = e; s.bo = o;
    for (int i = 0; i < MR_VECS; ++i) s.vec.emplace_back(s.n, s.m);
    s.part_a.assign(size_t(s.N), NAN);
    s.part_b.assign(size_t(s.N), NAN);
    std::memset(s.rec, 0xff, sizeof s.rec);
    s.first_block(0);
    s.second(0);
    for (int it = 1; it <= launched; ++it) {
        s.apply(it);
        s.first_block(it);
        s.second(it);
        if (s.rec[it & 1].status != MINRES_RUNNING) break;   // (frozen: the remaining launches write nothing but a copy of the record)
    }
}

// ---- what the entry points refuse (knot_ldl.h): 1 and the reason in msg, or 0 ---------------------------------------------------------------
int kbemu_factor_call_error(int hess, double floor, int factor, int pivots, int e, int o, int inertia, int status, char* msg, int msglen) {
    const char* r = kl_factor_call_error(hess, floor, factor, pivots, e, o, inertia, status);
    if (r) std::strncpy(msg, r, size_t(msglen - 1));
    return r != nullptr;
}
int kbemu_apply_call_error(int factor, int pivots, int e, int o, int minv_top, int minv_bottom, int r_top, int r_bottom, int z_top, int z_bottom, char* msg, int msglen) {
    const char* r = kl_apply_call_error(factor, pivots, e, o, minv_top, minv_bottom, r_top, r_bottom, z_top, z_bottom);
    if (r) std::strncpy(msg, r, size_t(msglen - 1));
    return r != nullptr;
}
int kbemu_minres_call_error(int hess, int jac, int factor, int pivots, int e, int o, int minv_top, int minv_bottom, int rhs_top, int rhs_bottom, int sol_top, int sol_bottom,
                            int iterations, int residual, int status, double rtol, int max_iterations, int check_every, char* msg, int msglen) {
    const char* r = kl_minres_call_error(hess, jac, factor, pivots, e, o, minv_top, minv_bottom, rhs_top, rhs_bottom, sol_top, sol_bottom, iterations, residual, status, rtol,
                                         max_iterations, check_every);
    if (r) std::strncpy(msg, r, size_t(msglen - 1));
    return r != nullptr;
}

}  // extern "C"
