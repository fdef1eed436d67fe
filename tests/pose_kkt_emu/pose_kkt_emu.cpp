// TEST-ONLY CPU emulation of the pose finder's KKT kernels (hipnlp_pose.hip hipnlp_pose_saddle_times_kernel, hipnlp_pose_saddle_diag_kernel,
// hipnlp_pose_saddle_solve_kernel): one workgroup of 256 "threads" per pose walked thread by thread, phase by phase, with the element
// expressions, the per-thread chains and the iteration steps of pose_kkt.h and knot_minres.h — the same headers the device compiles — and
// the tree of jprod_dot_tree.  The staging (what a workgroup holds in LDS) is stated here a second time, from the vectors of PoseLayout
// and not from PoseLayout::fill_kkt_tables: a word the device table gets wrong shows as a difference.  Every store goes through a counter.
// It is NOT part of the product: libhipnlp.so does not contain it.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../hippopt_amd/csrc/pose_kkt.h"
#include "../../hippopt_amd/csrc/pose_layout.h"

using namespace hipnlp;

namespace {

struct Handle {
    PoseLayout L;
    KinTables kt;
    PoseKktTables tables;   // the device tables, for the table test only
    // the staging of a workgroup in this file's own words
    std::vector<int32_t> cw, rw, tw, col_dir, row_dir, var_dir, hdiag;
};

void store(double* out, int* writes, int i, double v) { out[i] = v; writes[i]++; }

// what a workgroup stages of one pose: the value runs by CCS position (zeros behind them)
struct Pose {
    std::vector<double> jac, hess, vec;
    PoseKktStaged s;
    Pose(const Handle* h, const double* hess_values, const double* jac_values) : jac(PP_ENT_CAP, 0.0), hess(PK_HESS_CAP, 0.0), vec(PK_VEC_WORDS, 0.0) {
        for (int e = 0; e < h->L.nnz; ++e) jac[size_t(e)] = jac_values[e];
        for (int e = 0; e < h->L.hnnz; ++e) hess[size_t(e)] = hess_values[e];
        s = PoseKktStaged{jac.data(), hess.data(), h->cw.data(), h->rw.data(), h->tw.data()};
    }
};

// minv_top into mt [PK_WG] and minv_bottom into mb [PK_WG], one thread per variable, then one per row
void build_diagonal(const Handle* h, const Pose& p, const double* dx, const double* dc, double floor, double* mt, double* mb) {
    const int m = h->L.m;
    for (int tid = 0; tid < PK_WG; ++tid) {
        const int32_t hd = h->hdiag[size_t(tid)];
        mt[tid] = tid < POSE_NX ? pose_kkt_minv_top(dx != nullptr, hd >= 0 ? p.hess[size_t(hd)] : 0.0, dx ? dx[tid] : 0.0, floor) : 0.0;
    }
    for (int tid = 0; tid < PK_WG; ++tid)
        mb[tid] = tid < m ? pose_kkt_minv_bottom(p.s, h->row_dir[size_t(tid)], mt, dc != nullptr, dc ? dc[tid] : 0.0, floor) : 0.0;
}

}  // namespace

extern "C" {

Handle* pkemu_create(const hipnlp_pose_desc* desc, char* err, int errlen) {
    Handle* h = new Handle();
    std::string e;
    if (Layout::make_kin_tables(desc->model, h->kt, e)) Layout::fill_terrain_tops(h->kt, desc->settings.terrain, desc->settings.n_terrain_steps, desc->settings.terrain_steps);
    if (e.empty() && !h->L.build(desc->settings, h->kt)) e = h->L.error;
    if (e.empty() && !h->L.kkt_fits()) e = h->L.error;
    if (!e.empty()) {
        std::strncpy(err, e.c_str(), size_t(errlen - 1));
        delete h;
        return nullptr;
    }
    const PoseLayout& L = h->L;
    h->L.fill_kkt_tables(h->tables);
    h->cw.assign(PP_ENT_CAP, 0); h->rw.assign(PP_ENT_CAP, 0); h->tw.assign(PP_TOUCH_CAP, 0);
    h->col_dir.assign(PK_WG, 0); h->row_dir.assign(PK_WG, 0); h->var_dir.assign(PK_WG, 0); h->hdiag.assign(PK_WG, -1);
    for (int e2 = 0; e2 < L.nnz; ++e2) h->cw[size_t(e2)] = e2 | (L.irow[size_t(e2)] << PP_IDX_BITS);
    for (int q = 0; q < L.nnz; ++q) { const int e2 = L.jrowent[size_t(q)]; h->rw[size_t(q)] = e2 | (L.jcol[size_t(e2)] << PP_IDX_BITS); }
    for (size_t q = 0; q < L.htouch.size(); ++q) h->tw[q] = L.htouch[q].pos | (L.htouch[q].other << PP_IDX_BITS);
    for (int c = 0; c < POSE_NX; ++c) {
        h->col_dir[size_t(c)] = L.jcolptr[size_t(c)] | ((L.jcolptr[size_t(c) + 1] - L.jcolptr[size_t(c)]) << PP_IDX_BITS);
        h->var_dir[size_t(c)] = L.htouchptr[size_t(c)] | ((L.htouchptr[size_t(c) + 1] - L.htouchptr[size_t(c)]) << PP_IDX_BITS);
        h->hdiag[size_t(c)] = -1;
        for (int e2 = 0; e2 < L.hnnz; ++e2) if (L.hrow[size_t(e2)] == c && L.hcol[size_t(e2)] == c) h->hdiag[size_t(c)] = e2;
    }
    for (int r = 0; r < L.m; ++r) h->row_dir[size_t(r)] = L.jrowptr[size_t(r)] | ((L.jrowptr[size_t(r) + 1] - L.jrowptr[size_t(r)]) << PP_IDX_BITS);
    return h;
}
void pkemu_destroy(Handle* h) { delete h; }
void pkemu_dims(const Handle* h, int* n, int* m, int* nnz, int* hnnz) { *n = h->L.n; *m = h->L.m; *nnz = h->L.nnz; *hnnz = h->L.hnnz; }
void pkemu_sparsity(const Handle* h, int* irow, int* jcol, int* hrow, int* hcol) {
    for (int i = 0; i < h->L.nnz; ++i) { irow[i] = h->L.irow[size_t(i)]; jcol[i] = h->L.jcol[size_t(i)]; }
    for (int i = 0; i < h->L.hnnz; ++i) { hrow[i] = h->L.hrow[size_t(i)]; hcol[i] = h->L.hcol[size_t(i)]; }
}
// [0] entries of jac g, [1] rows, [2] touches, [3] entries of the Hessian, [4] threads, [5] iterations of one launch
void pkemu_caps(int* out) { out[0] = PP_ENT_CAP; out[1] = PP_ROW_CAP; out[2] = PP_TOUCH_CAP; out[3] = PK_HESS_CAP; out[4] = PK_WG; out[5] = PK_MAX_ITERATIONS; }
// the device tables (PoseLayout::fill_kkt_tables) and this file's own statement of them: col, row [PP_ENT_CAP], touch [PP_TOUCH_CAP], hdiag [PK_WG]
void pkemu_device_words(const Handle* h, int own, int* col_word, int* row_word, int* touch_word, int* hdiag) {
    std::memcpy(col_word, own ? h->cw.data() : h->tables.col_word, sizeof(h->tables.col_word));
    std::memcpy(row_word, own ? h->rw.data() : h->tables.row_word, sizeof(h->tables.row_word));
    std::memcpy(touch_word, own ? h->tw.data() : h->tables.touch_word, sizeof(h->tables.touch_word));
    std::memcpy(hdiag, own ? h->hdiag.data() : h->tables.hdiag, sizeof(h->tables.hdiag));
}
// the layout's own table (PoseLayout::hdiag [81])
void pkemu_hdiag(const Handle* h, int* out) { for (int c = 0; c < POSE_NX; ++c) out[c] = h->L.hdiag[size_t(c)]; }

// hipnlp_pose_saddle_times_kernel: [v | w] staged, thread t sums element t of the top and row t of the bottom
void pkemu_times(const Handle* h, const double* hess, const double* jac, const double* v, const double* w, const double* dx, const double* dc, double* top, int* top_writes,
                 double* bottom, int* bottom_writes) {
    Pose p(h, hess, jac);
    const int m = h->L.m;
    for (int tid = 0; tid < PK_WG; ++tid) {
        if (tid < POSE_NX) p.vec[size_t(tid)] = v[tid];
        if (tid < m) p.vec[size_t(PK_BOT + tid)] = w[tid];
    }
    for (int tid = 0; tid < PK_WG; ++tid) {
        if (tid < POSE_NX) store(top, top_writes, tid, pose_kkt_top(p.s, h->var_dir[size_t(tid)], h->col_dir[size_t(tid)], p.vec.data(), dx != nullptr, dx ? dx[tid] : 0.0, v[tid]));
        if (tid < m) store(bottom, bottom_writes, tid, pose_kkt_bottom(p.s, h->row_dir[size_t(tid)], p.vec.data(), dc != nullptr, dc ? dc[tid] : 0.0, w[tid]));
    }
}

// hipnlp_pose_saddle_diag_kernel
void pkemu_diag(const Handle* h, const double* hess, const double* jac, const double* dx, const double* dc, double floor, double* minv_top, int* top_writes, double* minv_bottom,
                int* bottom_writes) {
    Pose p(h, hess, jac);
    double mt[PK_WG], mb[PK_WG];
    build_diagonal(h, p, dx, dc, floor, mt, mb);
    for (int tid = 0; tid < PK_WG; ++tid) {
        if (tid < POSE_NX) store(minv_top, top_writes, tid, mt[tid]);
        if (tid < h->L.m) store(minv_bottom, bottom_writes, tid, mb[tid]);
    }
}

// hipnlp_pose_saddle_solve_kernel: the whole solve of one pose.  scalar_writes [3]: iterations, residual, status.  trace [maxit][3]
// (optional): alfa, beta, phibar of every iteration taken.
void pkemu_solve(const Handle* h, const double* hess, const double* jac, const double* rhs_top, const double* rhs_bottom, const double* dx, const double* dc,
                 const double* minv_top, const double* minv_bottom, int build_diag, double floor, double rtol, int maxit, double* sol_top, int* top_writes, double* sol_bottom,
                 int* bottom_writes, int* iterations, double* residual, int* status, int* scalar_writes, double* trace) {
    Pose p(h, hess, jac);
    const int m = h->L.m;
    double mt[PK_WG], mb[PK_WG];
    bool with_minv = minv_top != nullptr;
    for (int tid = 0; tid < PK_WG; ++tid) { mt[tid] = (with_minv && tid < POSE_NX) ? minv_top[tid] : 0.0; mb[tid] = (with_minv && tid < m) ? minv_bottom[tid] : 0.0; }
    if (build_diag) { build_diagonal(h, p, dx, dc, floor, mt, mb); with_minv = true; }
    PoseKktElem et[PK_WG], eb[PK_WG];
    double prod[PK_WG];
    auto has_top = [](int tid) { return tid < POSE_NX; };
    auto has_row = [m](int tid) { return tid < m; };
    for (int tid = 0; tid < PK_WG; ++tid) {
        pose_kkt_elem_start(et[tid], has_top(tid) ? rhs_top[tid] : 0.0, with_minv, mt[tid]);
        pose_kkt_elem_start(eb[tid], has_row(tid) ? rhs_bottom[tid] : 0.0, with_minv, mb[tid]);
        prod[tid] = pose_kkt_chain(has_top(tid), et[tid].r2, et[tid].y, has_row(tid), eb[tid].r2, eb[tid].y);
    }
    MinresRec rec = minres_init(jprod_dot_tree(prod), rtol, maxit);
    while (rec.status == MINRES_RUNNING) {
        for (int tid = 0; tid < PK_WG; ++tid) {
            pose_kkt_elem_v(et[tid], rec.beta);
            pose_kkt_elem_v(eb[tid], rec.beta);
            if (has_top(tid)) p.vec[size_t(tid)] = et[tid].v;
            if (has_row(tid)) p.vec[size_t(PK_BOT + tid)] = eb[tid].v;
        }
        const bool sub = rec.it >= 1;
        const double c1 = sub ? minres_div(rec.beta, rec.oldb) : 0.0;
        for (int tid = 0; tid < PK_WG; ++tid) {
            const double kt = has_top(tid) ? pose_kkt_top(p.s, h->var_dir[size_t(tid)], h->col_dir[size_t(tid)], p.vec.data(), dx != nullptr, dx ? dx[tid] : 0.0, et[tid].v) : 0.0;
            const double kb = has_row(tid) ? pose_kkt_bottom(p.s, h->row_dir[size_t(tid)], p.vec.data(), dc != nullptr, dc ? dc[tid] : 0.0, eb[tid].v) : 0.0;
            pose_kkt_elem_apply(et[tid], sub, c1, kt);
            pose_kkt_elem_apply(eb[tid], sub, c1, kb);
            prod[tid] = pose_kkt_chain(has_top(tid), et[tid].v, et[tid].y, has_row(tid), eb[tid].v, eb[tid].y);
        }
        const double alfa = jprod_dot_tree(prod);
        const double c2 = minres_div(alfa, rec.beta);
        for (int tid = 0; tid < PK_WG; ++tid) {
            pose_kkt_elem_residual(et[tid], c2, with_minv);
            pose_kkt_elem_residual(eb[tid], c2, with_minv);
            prod[tid] = pose_kkt_chain(has_top(tid), et[tid].r2, et[tid].y, has_row(tid), eb[tid].r2, eb[tid].y);
        }
        const double s = jprod_dot_tree(prod);
        MinresStep st;
        const MinresRec next = minres_step(rec, alfa, s, rtol, maxit, st);
        if (next.status != MINRES_BREAKDOWN)
            for (int tid = 0; tid < PK_WG; ++tid) { pose_kkt_elem_update(et[tid], st); pose_kkt_elem_update(eb[tid], st); }
        rec = next;
        if (trace && next.status != MINRES_BREAKDOWN) { double* t = trace + size_t(rec.it - 1) * 3; t[0] = rec.alfa; t[1] = rec.beta; t[2] = rec.phibar; }
    }
    for (int tid = 0; tid < PK_WG; ++tid) {
        if (has_top(tid)) store(sol_top, top_writes, tid, et[tid].z);
        if (has_row(tid)) store(sol_bottom, bottom_writes, tid, eb[tid].z);
        if (tid == 0) { *iterations = rec.it; *residual = rec.residual; *status = rec.status; for (int i = 0; i < 3; ++i) scalar_writes[i]++; }
    }
}

}  // extern "C"
