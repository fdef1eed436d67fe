// TEST-ONLY CPU emulation of hipnlp_kkt_minres_device (hipnlp.hip): the launches of the solve in their order — the start (first, second),
// then per iteration apply, first, second — each walked workgroup by workgroup over the knots of ONE trajectory, with the element-to-thread
// map (minres_owned), the per-thread chains, the tree (jprod_dot_tree), the per-knot partials, the double-buffered scalar records and
// every expression of knot_minres.h — the same header the device compiles.  y = K v is the emulation of the operator (tests/kkt_emu,
// compiled into this library as it stands).  It is NOT part of the product: libhipnlp.so does not contain it.
#include "../kkt_emu/kkt_emu.cpp"

#include "../../hippopt_amd/csrc/knot_minres.h"

namespace {

struct Vecs {
    std::vector<double> top, bottom;
    Vecs(int n, int m) : top(size_t(n), NAN), bottom(size_t(m), NAN) {}
};

struct Solve {
    const kktemu_handle* h;
    const double *hess, *jac, *dx, *dc, *minv_top, *minv_bottom, *rhs_top, *rhs_bottom;
    double *z_top, *z_bottom;
    int *z_top_writes, *z_bottom_writes, *scalar_writes;
    double rtol;
    int maxit, N, n, m;
    std::vector<Vecs> vec;
    std::vector<double> part_a, part_b;
    MinresRec rec[2];
    int* iterations;
    double* residual;
    int* status;

    const int32_t* row_a(int k) const { return h->T.row_a[h->L.pair_variant_of(k)]; }
    const int32_t* row_b(int k) const { return h->T.row_b[h->L.pair_variant_of(k)]; }

    // one workgroup's partial: chain(tid, owned) is the thread's fused multiply-add chain
    template <class Chain> double knot_partial(int k, const Chain& chain) const {
        double prod[JP_WG];
        for (int tid = 0; tid < JP_WG; ++tid) prod[tid] = chain(minres_owned(tid, k, N, row_a(k), row_b(k)));
        return jprod_dot_tree(prod);
    }

    void apply(int it) {
        const MinresRec& in = rec[(it - 1) & 1];
        if (in.status != MINRES_RUNNING) return;
        const bool sub = in.it >= 1;
        const double c1 = sub ? minres_div(in.beta, in.oldb) : 0.0;
        Vecs &v = vec[MR_V], &y = vec[MR_Y], &r1 = vec[MR_R1];
        std::vector<int> tw(size_t(n), 0), bw(size_t(m), 0);
        kktemu_times(h, hess, jac, dx, dc, v.top.data(), v.bottom.data(), y.top.data(), y.bottom.data(), tw.data(), bw.data());
        for (int k = 0; k < N; ++k)
            part_a[size_t(k)] = knot_partial(k, [&](const MinresOwned& o) {
                double acc = 0.0;
                if (o.top >= 0) { double& t = y.top[size_t(o.top)]; t = minres_sub_r1(sub, c1, sub ? r1.top[size_t(o.top)] : 0.0, t); acc = fm_fma(v.top[size_t(o.top)], t, acc); }
                for (int q = 0; q < 2; ++q)
                    if (o.row[q] >= 0) { double& t = y.bottom[size_t(o.row[q])]; t = minres_sub_r1(sub, c1, sub ? r1.bottom[size_t(o.row[q])] : 0.0, t); acc = fm_fma(v.bottom[size_t(o.row[q])], t, acc); }
                return acc;
            });
    }

    void first(int it) {
        const bool init = it == 0, with_minv = minv_top != nullptr;
        double c2 = 0.0;
        if (!init) {
            const MinresRec& in = rec[(it - 1) & 1];
            if (in.status != MINRES_RUNNING) return;
            c2 = minres_div(minres_sum(part_a.data(), N), in.beta);
        }
        auto element = [&](double& acc, int e, const double* rhs, const double* minv, std::vector<double> Vecs::*half, double* z, int* zw) {
            if (e < 0) return;
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
            const double ym = minres_precond(with_minv, with_minv ? minv[i] : 0.0, r);
            (vec[MR_Y].*half)[i] = ym;
            acc = fm_fma(r, ym, acc);
        };
        for (int k = 0; k < N; ++k)
            part_b[size_t(k)] = knot_partial(k, [&](const MinresOwned& o) {
                double acc = 0.0;
                element(acc, o.top, rhs_top, minv_top, &Vecs::top, z_top, z_top_writes);
                for (int q = 0; q < 2; ++q) element(acc, o.row[q], rhs_bottom, minv_bottom, &Vecs::bottom, z_bottom, z_bottom_writes);
                return acc;
            });
    }

    void second(int it) {
        const bool init = it == 0;
        const MinresRec in = rec[(it - 1) & 1];
        MinresRec& out = rec[it & 1];
        for (int k = 0; k < N; ++k) {   // every workgroup takes the scalar step itself
            MinresRec r;
            MinresStep st = {0.0, 0.0, 0.0, 0.0};
            bool update = false;
            if (init) {
                r = minres_init(minres_sum(part_b.data(), N), rtol, maxit);
            } else {
                if (in.status != MINRES_RUNNING) {
                    if (k == 0) out = in;
                    continue;
                }
                r = minres_step(in, minres_sum(part_a.data(), N), minres_sum(part_b.data(), N), rtol, maxit, st);
                update = r.status != MINRES_BREAKDOWN;
            }
            if (k == 0) {
                out = r;
                *iterations = r.it; *residual = r.residual; *status = r.status;
                for (int i = 0; i < 3; ++i) scalar_writes[i]++;
            }
            const bool next = r.status == MINRES_RUNNING;
            if (!update && !next) continue;
            auto element = [&](int e, std::vector<double> Vecs::*half, double* z, int* zw) {
                if (e < 0) return;
                const size_t i = size_t(e);
                if (update) {
                    const double w1 = (vec[MR_W2].*half)[i], wo = (vec[MR_W].*half)[i];
                    const double wn = minres_new_w(st, (vec[MR_V].*half)[i], w1, wo);
                    (vec[MR_W2].*half)[i] = wo;
                    (vec[MR_W].*half)[i] = wn;
                    z[i] = minres_new_z(st, wn, z[i]); zw[i]++;
                }
                if (next) (vec[MR_V].*half)[i] = minres_div((vec[MR_Y].*half)[i], r.beta);
            };
            for (int tid = 0; tid < JP_WG; ++tid) {
                const MinresOwned o = minres_owned(tid, k, N, row_a(k), row_b(k));
                element(o.top, &Vecs::top, z_top, z_top_writes);
                for (int q = 0; q < 2; ++q) element(o.row[q], &Vecs::bottom, z_bottom, z_bottom_writes);
            }
        }
    }
};

}  // namespace

extern "C" {

// One trajectory: the start and `launched` iterations' launches (what hipnlp_kkt_minres_device enqueues with check_every == 0 is
// launched == maxit).  sol_top [n] / sol_bottom [m], iterations, residual, status: the outputs; *_writes count the stores to them
// (scalar_writes [3]: iterations, residual, status).  trace [launched][6] (optional): per iteration alfa, beta, phibar, status, the record's
// it, and whether the trajectory was still running when the iteration began.  trace_vec [launched][4][n + m] (optional): v, y as alfa
// sees it (K v - (beta/oldb) r1), the new r2 and M^-1 r2 of every iteration that ran.
void kmremu_solve(const kktemu_handle* h, const double* hess, const double* jac, const double* dx, const double* dc, const double* minv_top, const double* minv_bottom,
                  const double* rhs_top, const double* rhs_bottom, double* sol_top, double* sol_bottom, double rtol, int maxit, int launched, int* iterations, double* residual,
                  int* status, int* top_writes, int* bottom_writes, int* scalar_writes, double* trace, double* trace_vec) {
    Solve s;
    s.h = h; s.hess = hess; s.jac = jac; s.dx = dx; s.dc = dc; s.minv_top = minv_top; s.minv_bottom = minv_bottom; s.rhs_top = rhs_top; s.rhs_bottom = rhs_bottom;
    s.z_top = sol_top; s.z_bottom = sol_bottom; s.z_top_writes = top_writes; s.z_bottom_writes = bottom_writes; s.scalar_writes = scalar_writes;
    s.rtol = rtol; s.maxit = maxit; s.N = h->L.N; s.n = h->L.n; s.m = h->L.m;
    s.iterations = iterations; s.residual = residual; s.status = status;
    for (int i = 0; i < MR_VECS; ++i) s.vec.emplace_back(s.n, s.m);
    s.part_a.assign(size_t(s.N), NAN);
    s.part_b.assign(size_t(s.N), NAN);
    std::memset(s.rec, 0xff, sizeof s.rec);
    s.first(0);
    s.second(0);
    const size_t nm = size_t(s.n) + size_t(s.m);
    auto dump = [&](double* dst, const Vecs& v) { std::memcpy(dst, v.top.data(), sizeof(double) * size_t(s.n)); std::memcpy(dst + s.n, v.bottom.data(), sizeof(double) * size_t(s.m)); };
    for (int it = 1; it <= launched; ++it) {
        const bool ran = s.rec[(it - 1) & 1].status == MINRES_RUNNING;
        double* tv = (trace_vec && ran) ? trace_vec + size_t(it - 1) * 4 * nm : nullptr;
        if (tv) dump(tv, s.vec[MR_V]);
        s.apply(it);
        if (tv) dump(tv + nm, s.vec[MR_Y]);
        s.first(it);
        if (tv) { dump(tv + 2 * nm, s.vec[MR_R2]); dump(tv + 3 * nm, s.vec[MR_Y]); }
        s.second(it);
        if (trace) {
            const MinresRec& r = s.rec[it & 1];
            double* t = trace + size_t(it - 1) * 6;
            t[0] = r.alfa; t[1] = r.beta; t[2] = r.phibar; t[3] = r.status; t[4] = r.it; t[5] = ran ? 1.0 : 0.0;
        }
    }
}

}  // extern "C"
