// TEST-ONLY CPU emulation of the pose finder's product kernels (hipnlp_pose.hip hipnlp_pose_lgrad_kernel, hipnlp_pose_jvp_kernel,
// hipnlp_pose_hvp_kernel): the pose program on the DEVICE emitter's cut Jacobian staging (pose_body.h pjs) and the pose Hessian program, as
// tests/hostemu runs them, then the sums of pose_products.h over the device tables of PoseLayout::fill_product_tables — the same header,
// the same words, one "thread" at a time.  Every store goes through a counter.
// It is NOT part of the product: libhipnlp.so does not contain it.
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "../../hippopt_amd/csrc/pose_layout.h"

using namespace hipnlp;

namespace {

long g_map_violations = 0;
int g_wave_order = -1;

// (hipnlp_pose.hip PoseEm: J indexes a pointer moved back by a constant, JC / JD map any kept slot)
struct StagedEm {
    static constexpr int kTerrain = -1;
    double* g;
    double* stg;
    void G(int slot, int, double v) { g[slot] = v; }
    void J(int slot, int, int, double v) { if (slot < js::V0) { g_map_violations++; return; } stg[pjs::index(slot)] = v; }
    void JC(int slot, int, int, double v) { if (!pjs::kept(slot)) { g_map_violations++; return; } stg[pjs::index(slot)] = v; }
    void JD(int slot, int, int, double v) { JC(slot, 0, 0, v); }
};
struct HessEm {
    static constexpr int kTerrain = -1;
    double* g;
    double* jac;
    double* hess;
    void G(int slot, int, double v) { g[slot] = v; }
    void J(int slot, int, int, double v) { jac[slot] = v; }
    void H(int slot, int, int, double v) { hess[slot] = v; }
};

// the groups of a phase collected in table order, run wave by wave in a permuted order of the four waves
struct WaveOrder {
    int waves, order;
    std::vector<std::pair<int, std::function<void()>>> groups;
    void add(int w, std::function<void()> fn) { groups.push_back({w, std::move(fn)}); }
    void flush() {
        for (int q = 0; q < waves; ++q) {
            const int w = order == 0 ? q : (order == 1 ? waves - 1 - q : (q + waves / 2) % waves);
            for (auto& gq : groups) if (gq.first == w) gq.second();
        }
        groups.clear();
    }
};

struct Handle {
    hipnlp_pose_desc d;
    KinTables kt;
    KSettings ks;
    PoseHands hands;
    PoseLayout L;
    PoseProdTables pt;
};

void load_scratch(KnotScratch* s, const double* x, const double* p, GParams& gp) {
    double pk[PK_STRIDE], xr[64];
    pack_pose_params(p, pk, xr, gp);
    std::fill(reinterpret_cast<double*>(s), reinterpret_cast<double*>(s) + sizeof(KnotScratch) / sizeof(double), std::nan(""));
    for (int i = 0; i < XPAD; ++i) { s->x[i] = 0; s->xm[i] = 0; }
    for (int i = 0; i < NPER; ++i) s->xo[i] = 0;
    for (int i = 0; i < POSE_NX; ++i) s->x[pose_to_knot_col(i)] = x[i];
    for (int i = 0; i < 64; ++i) s->xm[i] = xr[i];
    for (int i = 0; i < PK_STRIDE; ++i) s->pk[i] = pk[i];
}

// the pose program as hipnlp_pose_kernel runs it: values of jac g in the cut staging `stg`, grad f and g in the scratch
void run_pose_program(const Handle* h, const double* x, const double* p, KnotScratch* s, std::vector<double>& stg) {
    GParams gp;
    load_scratch(s, x, p, gp);
    stg.assign(size_t(pjs::slots(false)), std::nan(""));   // (the larger of the two terrains' stagings)
    KnotInfo ki{1, 3, 0, 0};
    StagedEm em{s->g, stg.data()};
    Ctx<StagedEm> cx(*s, h->kt, h->ks, gp, ki, em);
    cx.hands = &h->hands;
    if (g_wave_order < 0) {
#define HOST_R(w4, w8, fn, nt) for (int t_ = 0; t_ < (nt); ++t_) fn(cx, t_);
        HIPNLP_POSE_PROGRAM(HOST_R, )
#undef HOST_R
    } else {
        WaveOrder wo{4, g_wave_order, {}};
#define HOST_R(w4, w8, fn, nt) wo.add((w4), [&cx]() { for (int t_ = 0; t_ < (nt); ++t_) fn(cx, t_); });
#define HOST_BARRIER wo.flush();
        HIPNLP_POSE_PROGRAM(HOST_R, HOST_BARRIER)
#undef HOST_R
#undef HOST_BARRIER
        wo.flush();
    }
}

// the pose Hessian program as hipnlp_pose_hess_kernel runs it (multipliers: row i to the native slot of row i, over zeros)
void run_hess_program(const Handle* h, const double* x, const double* p, double sigma, const double* lambda, KnotScratch* s, HessScratch* hx) {
    const PoseLayout& L = h->L;
    GParams gp;
    load_scratch(s, x, p, gp);
    std::fill(reinterpret_cast<double*>(hx), reinterpret_cast<double*>(hx) + sizeof(HessScratch) / sizeof(double), std::nan(""));
    for (int slot = 0; slot < gs::COUNT; ++slot) hx->lam[slot] = 0.0;
    for (int slot = 0; slot < gs::COUNT; ++slot) if (L.g_row[size_t(slot)] >= 0) hx->lam[slot] = lambda[L.g_row[size_t(slot)]];
    hx->sigma = sigma;
    KnotInfo ki{1, 3, 0, 0};
    HessEm em{s->g, s->jac, hx->H};
    Ctx<HessEm> cx(*s, h->kt, h->ks, gp, ki, em);
    cx.hands = &h->hands;
    HCtx<HessEm> hcx{cx, *hx};
    if (g_wave_order < 0) {
#define HOST_KIN(w, fn, nt) for (int t_ = 0; t_ < (nt); ++t_) fn(cx, t_);
#define HOST_RH(w, fn, nt) for (int t_ = 0; t_ < (nt); ++t_) fn(hcx, t_);
        HIPNLP_POSE_HESS_PROGRAM(HOST_KIN, HOST_RH, )
#undef HOST_KIN
#undef HOST_RH
    } else {
        WaveOrder wo{4, g_wave_order, {}};
#define HOST_KIN(w, fn, nt) wo.add((w), [&cx]() { for (int t_ = 0; t_ < (nt); ++t_) fn(cx, t_); });
#define HOST_RH(w, fn, nt) wo.add((w), [&hcx]() { for (int t_ = 0; t_ < (nt); ++t_) fn(hcx, t_); });
#define HOST_BARRIER wo.flush();
        HIPNLP_POSE_HESS_PROGRAM(HOST_KIN, HOST_RH, HOST_BARRIER)
#undef HOST_KIN
#undef HOST_RH
#undef HOST_BARRIER
        wo.flush();
    }
}

void store(double* out, int* writes, int i, double v) { out[i] = v; writes[i]++; }

}  // namespace

extern "C" {

Handle* ppemu_create(const hipnlp_pose_desc* desc, char* err, int errlen) {
    Handle* h = new Handle();
    h->d = *desc;
    std::string e;
    if (Layout::make_kin_tables(desc->model, h->kt, e)) Layout::fill_terrain_tops(h->kt, desc->settings.terrain, desc->settings.n_terrain_steps, desc->settings.terrain_steps);
    if (!e.empty() || !h->L.build(desc->settings, h->kt)) {
        if (e.empty()) e = h->L.error;
        std::strncpy(err, e.c_str(), size_t(errlen - 1));
        delete h;
        return nullptr;
    }
    h->ks = PoseLayout::make_ksettings(desc->settings);
    h->hands = PoseLayout::make_hands(desc->settings);
    h->L.fill_product_tables(h->pt);
    return h;
}
void ppemu_destroy(Handle* h) { delete h; }
void ppemu_set_wave_order(int order) { g_wave_order = order; }
long ppemu_map_violations(void) { return g_map_violations; }
void ppemu_dims(const Handle* h, int* n, int* m, int* nnz, int* hnnz, int* ntouch) {
    *n = h->L.n; *m = h->L.m; *nnz = h->L.nnz; *hnnz = h->L.hnnz; *ntouch = int(h->L.htouch.size());
}
// [0] entries of jac g, [1] rows, [2] touches, [3] entries of one column / row / variable, [4] threads of a workgroup
void ppemu_caps(int* out) { out[0] = PP_ENT_CAP; out[1] = PP_ROW_CAP; out[2] = PP_TOUCH_CAP; out[3] = PP_CNT_MAX; out[4] = PP_WG; }
void ppemu_sparsity(const Handle* h, int* irow, int* jcol, int* hrow, int* hcol) {
    for (int i = 0; i < h->L.nnz; ++i) { irow[i] = h->L.irow[size_t(i)]; jcol[i] = h->L.jcol[size_t(i)]; }
    for (int i = 0; i < h->L.hnnz; ++i) { hrow[i] = h->L.hrow[size_t(i)]; hcol[i] = h->L.hcol[size_t(i)]; }
}
// the directories of PoseLayout::build_product_tables
void ppemu_tables(const Handle* h, int* jcolptr, int* jrowptr, int* jrowent, int* htouchptr, int* tpos, int* tslot, int* tother) {
    const PoseLayout& L = h->L;
    for (size_t i = 0; i < L.jcolptr.size(); ++i) jcolptr[i] = L.jcolptr[i];
    for (size_t i = 0; i < L.jrowptr.size(); ++i) jrowptr[i] = L.jrowptr[i];
    for (size_t i = 0; i < L.jrowent.size(); ++i) jrowent[i] = L.jrowent[i];
    for (size_t i = 0; i < L.htouchptr.size(); ++i) htouchptr[i] = L.htouchptr[i];
    for (size_t i = 0; i < L.htouch.size(); ++i) { tpos[i] = L.htouch[i].pos; tslot[i] = L.htouch[i].slot; tother[i] = L.htouch[i].other; }
}
// the device words (what the kernels read): PP_ENT_CAP + PP_ENT_CAP + PP_TOUCH_CAP + 3 * PP_WG
void ppemu_device_words(const Handle* h, int* col_word, int* row_word, int* touch_word, int* col_dir, int* row_dir, int* var_dir) {
    std::memcpy(col_word, h->pt.col_word, sizeof(h->pt.col_word));
    std::memcpy(row_word, h->pt.row_word, sizeof(h->pt.row_word));
    std::memcpy(touch_word, h->pt.touch_word, sizeof(h->pt.touch_word));
    std::memcpy(col_dir, h->pt.col_dir, sizeof(h->pt.col_dir));
    std::memcpy(row_dir, h->pt.row_dir, sizeof(h->pt.row_dir));
    std::memcpy(var_dir, h->pt.var_dir, sizeof(h->pt.var_dir));
}
// native Hessian slot of every CCS position (hperm), staging index of every CCS position of jac g
void ppemu_perms(const Handle* h, int* jstage, int* hperm) {
    for (int e = 0; e < h->L.nnz; ++e) jstage[e] = pjs::index(h->L.jperm[size_t(e)]);
    for (int e = 0; e < h->L.hnnz; ++e) hperm[e] = h->L.hperm[size_t(e)];
}

// the copy-out of hipnlp_pose_kernel (the "same source" of the first-order checks)
void ppemu_eval(const Handle* h, const double* x, const double* p, double* f, double* grad, double* g, double* jac) {
    const PoseLayout& L = h->L;
    KnotScratch* s = new KnotScratch();
    std::vector<double> stg;
    run_pose_program(h, x, p, s, stg);
    for (int e = 0; e < L.nnz; ++e) jac[e] = stg[size_t(pjs::index(L.jperm[size_t(e)]))];
    for (int slot = 0; slot < gs::COUNT; ++slot) if (L.g_row[size_t(slot)] >= 0) g[L.g_row[size_t(slot)]] = s->g[slot];
    for (int i = 0; i < POSE_NX; ++i) grad[i] = s->grad[pose_to_knot_col(i)];
    *f = s->cost[CT_POSE_TOTAL];
    delete s;
}
// the copy-out of hipnlp_pose_hess_kernel (the "same source" of the second-order checks)
void ppemu_hess(const Handle* h, const double* x, const double* p, double sigma, const double* lambda, double* hess) {
    KnotScratch* s = new KnotScratch();
    HessScratch* hx = new HessScratch();
    run_hess_program(h, x, p, sigma, lambda, s, hx);
    for (int e = 0; e < h->L.hnnz; ++e) hess[e] = hx->H[h->L.hperm[size_t(e)]];
    delete hx;
    delete s;
}

// hipnlp_pose_lgrad_kernel: factors (thread i: the multiplier of row i) and entry words staged, one thread per column
void ppemu_lgrad(const Handle* h, const double* x, const double* p, double sigma, const double* lambda, double* out, int* writes) {
    KnotScratch* s = new KnotScratch();
    std::vector<double> stg;
    run_pose_program(h, x, p, s, stg);
    double fs[PP_WG];
    std::vector<int32_t> ws(PP_ENT_CAP);
    for (int tid = 0; tid < PP_WG; ++tid) {
        fs[tid] = tid < h->L.m ? lambda[tid] : 0.0;
        for (int it = 0; it < PP_ENT_CAP / PP_WG; ++it) ws[size_t(tid + it * PP_WG)] = h->pt.col_word[tid + it * PP_WG];
    }
    for (int tid = 0; tid < PP_WG; ++tid)
        if (tid < POSE_NX) store(out, writes, tid, pose_xbar_column(sigma, s->grad[pose_to_knot_col(tid)], h->pt.col_dir[tid], ws.data(), fs, stg.data()));
    delete s;
}
// hipnlp_pose_jvp_kernel: factors (thread i: element i of v) and the words of the row directory staged, one thread per row, one lane for grad f . v
void ppemu_jvp(const Handle* h, const double* x, const double* p, const double* v, double* dot, int* dot_writes, double* jv, int* jv_writes) {
    KnotScratch* s = new KnotScratch();
    std::vector<double> stg;
    run_pose_program(h, x, p, s, stg);
    double fs[PP_WG];
    std::vector<int32_t> ws(PP_ENT_CAP);
    for (int tid = 0; tid < PP_WG; ++tid) {
        fs[tid] = tid < POSE_NX ? v[tid] : 0.0;
        for (int it = 0; it < PP_ENT_CAP / PP_WG; ++it) ws[size_t(tid + it * PP_WG)] = h->pt.row_word[tid + it * PP_WG];
    }
    for (int tid = 0; tid < PP_WG; ++tid) {
        const double y = pose_jv_row(h->pt.row_dir[tid], ws.data(), fs, stg.data());
        const double d = tid == PP_WG - 1 ? pose_gradf_dot_v(s->grad, fs) : 0.0;
        if (jv && tid < h->L.m) store(jv, jv_writes, tid, y);
        if (dot && tid == PP_WG - 1) store(dot, dot_writes, 0, d);
    }
    delete s;
}
// hipnlp_pose_hvp_kernel: touch words and v staged, one thread per variable over hx.H
void ppemu_hvp(const Handle* h, const double* x, const double* p, double sigma, const double* lambda, const double* v, double* out, int* writes) {
    KnotScratch* s = new KnotScratch();
    HessScratch* hx = new HessScratch();
    run_hess_program(h, x, p, sigma, lambda, s, hx);
    double vs[PP_WG];
    std::vector<int32_t> ws(PP_TOUCH_CAP);
    for (int tid = 0; tid < PP_WG; ++tid) {
        vs[tid] = tid < POSE_NX ? v[tid] : 0.0;
        for (int it = 0; it < PP_TOUCH_CAP / PP_WG; ++it) ws[size_t(tid + it * PP_WG)] = h->pt.touch_word[tid + it * PP_WG];
    }
    for (int tid = 0; tid < PP_WG; ++tid)
        if (tid < POSE_NX) store(out, writes, tid, pose_hv_row(h->pt.var_dir[tid], ws.data(), vs, hx->H));
    delete hx;
    delete s;
}

}  // extern "C"
