// knot_minres.h — preconditioned MINRES (Paige and Saunders) on the KKT operator of knot_kkt.h, for every trajectory of a batch at once
// (hipnlp.hip hipnlp_kkt_minres_device; the test-only CPU emulation tests/kkt_minres_emu runs the same text):
//
//     K [z_top; z_bottom] = [b_top; b_bottom],   K = [[H + diag d_x, J^T], [J, -diag d_c]],   M^-1 = diag(minv) > 0 (or the identity)
//
//     r1 = r2 = b;  y = M^-1 r2;  beta1 = beta = sqrt(r2.y);  oldb = dbar = epsln = 0;  phibar = beta1;  cs = -1;  sn = 0;  w = w2 = 0;  z = 0
//     iteration it = 1, 2, ...:
//       v = y / beta;  y = K v;  if it >= 2: y -= (beta/oldb) r1
//       alfa = v.y;  y -= (alfa/beta) r2;  r1 = r2;  r2 = y;  y = M^-1 r2;  oldb = beta;  beta = sqrt(r2.y)
//       oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta;  dbar = -cs beta
//       gamma = max(sqrt(gbar^2 + beta^2), DBL_MIN);  cs = gbar/gamma;  sn = beta/gamma;  phi = cs phibar;  phibar = sn phibar
//       w1 = w2;  w2 = w;  w = (v - oldeps w1 - delta w2)/gamma;  z += phi w
//       stop when phibar <= rtol beta1
//
// No workgroup waits for another one, there are no atomics and no persistent kernel: every reduction over a trajectory crosses a LAUNCH
// boundary.  One iteration is three launches on the grid (knots, batch) of the operator:
//   apply   y = K v as hipnlp_kkt_times_kernel sums it, then y -= (beta/oldb) r1 (it >= 2) by one fused multiply-add per element, and the
//           knot's partial of v.y;
//   first   every workgroup adds the N partials of its trajectory (minres_sum: from +0.0 in ascending knot order — the same bits in every
//           workgroup, at every N: there is no separate reduce launch, also beyond 256 knots), then y, r1, r2 and M^-1 r2 for the elements
//           it owns and the knot's partial of r2.y;
//   second  every workgroup adds both runs of partials and takes the scalar step (minres_step) redundantly, updates w2, w and z and writes
//           the next v for the elements it owns; the workgroup of knot 0 writes the trajectory's new scalar record and the three
//           per-trajectory outputs.
// The start is the `first` and the `second` launch in their initial form (r2 = b in place of the recurrence; minres_init).
// The scalar records are double-buffered by iteration parity: the launches of iteration it read record (it - 1) & 1, the workgroup of
// knot 0 writes record it & 1.  A trajectory with a final status is FROZEN: its workgroups return before they write anything but a copy
// of the record into the other buffer.
//
// What a knot owns (minres_owned): thread tid < NXK the element NXK k + tid of the top, the last knot's threads JP_V_STRIDE .. (the
// operator's LG_SPAN_GLOB) the six horizon-global elements, and thread tid the rows JprodTables::row_a / row_b [tid] and [tid + JP_WG] of the bottom — the elements whose
// K v that workgroup of the operator writes.  A per-knot partial of a . b: per thread ONE chain acc = fma(a_e, b_e, acc) from +0.0 over
// its top element, then its first, then its second row (a thread without an element keeps +0.0); then jprod_dot_tree over the 256 threads.
#pragma once
#include <cfloat>
#include <cmath>

#include "knot_jprod.h"

namespace hipnlp {

enum MinresStatus : int32_t { MINRES_RUNNING = -1, MINRES_CONVERGED = 0, MINRES_ITERATION_LIMIT = 1, MINRES_BREAKDOWN = 2 };

// correctly rounded on both sides, whatever the compiler's fast paths
HD double minres_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
HD double minres_sqrt(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(a);
#else
    return std::sqrt(a);
#endif
}
HD bool minres_finite(double a) { return a - a == 0.0; }

// the scalars of one trajectory between two iterations
struct MinresRec {
    double beta1, beta, oldb, dbar, epsln, phibar, cs, sn;
    double alfa;        // of the last iteration taken (0 before the first): not read by the recurrence
    double residual;    // phibar / beta1 (0 with beta1 == 0; 1 for a breakdown at the start: z = 0)
    int32_t it, status;
};
// what the vector update of an iteration needs besides the record
struct MinresStep { double oldeps, delta, gamma, phi; };

// the vectors of the workspace, each [batch][n] followed by [batch][m]
enum MinresVec : int { MR_V = 0, MR_Y = 1, MR_R1 = 2, MR_R2 = 3, MR_W = 4, MR_W2 = 5, MR_VECS = 6 };

// the partials of one trajectory, from +0.0 in ascending knot order
HD double minres_sum(const double* part, int N) {
    double acc = 0.0;
    for (int k = 0; k < N; ++k) acc += part[k];
    return acc;
}

HD int32_t minres_status_of(double phibar, double beta1, double rtol, int it, int maxit) {
    return phibar <= rtol * beta1 ? MINRES_CONVERGED : (it >= maxit ? MINRES_ITERATION_LIMIT : MINRES_RUNNING);
}

// the start: s = b . M^-1 b
HD MinresRec minres_init(double s, double rtol, int maxit) {
    MinresRec r;
    r.beta1 = r.beta = r.oldb = r.dbar = r.epsln = r.phibar = r.sn = r.alfa = 0.0;
    r.cs = -1.0;
    r.residual = 1.0;
    r.it = 0;
    if (!(s >= 0.0) || !minres_finite(s)) { r.status = MINRES_BREAKDOWN; return r; }   // M is not positive definite, or b is not finite
    r.beta1 = r.beta = r.phibar = minres_sqrt(s);
    if (r.beta1 == 0.0) { r.residual = 0.0; r.status = MINRES_CONVERGED; return r; }
    r.status = minres_status_of(r.phibar, r.beta1, rtol, 0, maxit);
    return r;
}

// one iteration's scalars: alfa = v . y, s = r2 . M^-1 r2 of the NEW r2.  A breakdown returns the old record with status 2 (and st is
// not to be used): the vectors stay as they are.
HD MinresRec minres_step(const MinresRec& in, double alfa, double s, double rtol, int maxit, MinresStep& st) {
    MinresRec r = in;
    st.oldeps = st.delta = st.gamma = st.phi = 0.0;
    if (!(s >= 0.0) || !minres_finite(s) || !minres_finite(alfa)) { r.status = MINRES_BREAKDOWN; return r; }
    const double beta = minres_sqrt(s);
    st.oldeps = in.epsln;
    st.delta = fm_fma(in.cs, in.dbar, in.sn * alfa);
    const double gbar = fm_fma(in.sn, in.dbar, -(in.cs * alfa));
    const double g = minres_sqrt(fm_fma(gbar, gbar, beta * beta));
    if (!minres_finite(g)) { r.status = MINRES_BREAKDOWN; return r; }
    st.gamma = g < DBL_MIN ? DBL_MIN : g;
    r.alfa = alfa;
    r.oldb = in.beta;
    r.beta = beta;
    r.epsln = in.sn * beta;
    r.dbar = -(in.cs * beta);
    r.cs = minres_div(gbar, st.gamma);
    r.sn = minres_div(beta, st.gamma);
    st.phi = r.cs * in.phibar;
    r.phibar = r.sn * in.phibar;
    r.residual = minres_div(r.phibar, in.beta1);
    r.it = in.it + 1;
    r.status = minres_status_of(r.phibar, in.beta1, rtol, r.it, maxit);
    return r;
}

// the element-wise expressions, one text for both sides
// apply: y = (K v)_e - (beta/oldb) r1_e from the second iteration on
HD double minres_sub_r1(bool sub, double c1, double r1, double kv) { return sub ? fm_fma(-c1, r1, kv) : kv; }
// first: r2_new = y - (alfa/beta) r2
HD double minres_new_r2(double c2, double r2, double y) { return fm_fma(-c2, r2, y); }
HD double minres_precond(bool with_minv, double minv, double r2) { return with_minv ? minv * r2 : r2; }
// second: w_new = (v - oldeps w1 - delta w2) / gamma with w1 = the old w2 and w2 = the old w;  z += phi w_new
HD double minres_new_w(const MinresStep& st, double v, double w1, double w2) { return minres_div(fm_fma(-st.delta, w2, fm_fma(-st.oldeps, w1, v)), st.gamma); }
HD double minres_new_z(const MinresStep& st, double w, double z) { return fm_fma(st.phi, w, z); }

// what thread tid of knot k's workgroup owns: an element of the top (-1: none) and two rows of the bottom (-1: none); row_a / row_b are
// the JP_ROW_CAP words of the knot's pair variant
struct MinresOwned { int32_t top, row[2]; };
HD MinresOwned minres_owned(int tid, int k, int N, const int32_t* row_a, const int32_t* row_b) {
    MinresOwned o;
    o.top = tid < NXK ? NXK * k + tid : ((k == N - 1 && tid >= JP_V_STRIDE && tid < JP_V_STRIDE + NXG) ? NXK * N + (tid - JP_V_STRIDE) : -1);
    for (int it = 0; it < 2; ++it) {
        const int32_t ra = row_a[tid + it * JP_WG];
        o.row[it] = ra != G_NONE ? ra + row_b[tid + it * JP_WG] * k : -1;
    }
    return o;
}
static_assert(JP_ROW_CAP == 2 * JP_WG && NXK <= JP_V_STRIDE && JP_V_STRIDE + NXG <= JP_WG, "one element of the top and two rows per thread");

}  // namespace hipnlp
