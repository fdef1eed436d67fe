// pose_kkt.h — the KKT chain of the static pose finder from STORED value runs (hipnlp_pose.hip hipnlp_pose_saddle_times_kernel,
// hipnlp_pose_saddle_diag_kernel, hipnlp_pose_saddle_solve_kernel; the test-only CPU emulation tests/pose_kkt_emu runs the same text):
//
//     K [v; w] = [ (H + diag d_x) v + J^T w ]   top     [81]        the operator           (knot_kkt.h's combinations)
//                [  J v - diag(d_c) w       ]   bottom  [m]
//     M^-1     = diag(minv_top, minv_bottom) > 0                    the diagonal           (knot_kkt_precond.h's arithmetic)
//     K z = b  by preconditioned MINRES from a zero start            the solve              (knot_minres.h's recurrence, unchanged)
//
// H and J are the value runs hipnlp_pose_eval_hess_device (lower triangle, CCS order) and hipnlp_pose_eval_device (jac g, CCS order) of
// the same handle wrote; no pose program runs here.  A pose is ONE workgroup of 256 threads: both runs, the three word tables and a vector
// record fit in 31 KB of LDS, thread t owns element t of the top (t < 81) and row t of the bottom (t < m), and every reduction of MINRES is
// a tree over the workgroup.  So a whole solve — up to max_iterations iterations — is ONE launch per batch of poses: no workspace in
// memory, no scalar leaves the CU, no workgroup waits for another one.  y, r1, r2, w, w2, z (and v, minv) of a thread's two elements stay
// in registers (PoseKktElem); only v goes through LDS, for the operator.
//
// The sums, each one chain from +0.0 of one fused multiply-add per entry:
//   hv_c  pose_hv_row over the touches of variable c in table order (CCS-position order);
//   jt_c  the column sum over the CCS positions of column c in order, no gradient term (pose_xbar_column with sigma = grad = 0);
//   jv_i  pose_jv_row over the entries of row i in ascending column.
// A dot product a . b: per thread ONE chain fma(a_top, b_top, +0.0), then fma(a_row, b_row, acc) (a thread without an element keeps
// +0.0), then the tree of jprod_dot_tree over the 256 threads.  Every thread takes the same sum from LDS and runs minres_init /
// minres_step itself: the scalars and the loop exit are the same in every thread of the workgroup, which the barriers inside the loop need.
#pragma once
#include <cstdint>

#include "knot_kkt.h"
#include "knot_kkt_precond.h"
#include "knot_minres.h"
#include "pose_products.h"

namespace hipnlp {

// What a workgroup stages: the caps of pose_products.h for the entries of jac g, the rows and the touches, and three words per thread
// for the lower triangle of the Hessian (373 .. 485 entries by variant).  PoseLayout::kkt_fits checks a handle's pattern against them.
constexpr int PK_WG = PP_WG;
constexpr int PK_HESS_CAP = 3 * PK_WG;
// the vector record of the operator: elements of the top at [0, 81), of the bottom at [PK_BOT, PK_BOT + m)
constexpr int PK_BOT = 128;
constexpr int PK_VEC_WORDS = PK_BOT + PP_ROW_CAP;
// one launch runs at most this many iterations (a bound on one launch, not on the method)
constexpr int PK_MAX_ITERATIONS = 4096;
static_assert(POSE_NX <= PK_BOT && PK_HESS_CAP <= (1 << PP_IDX_BITS) && PP_ROW_CAP == PK_WG, "one element of the top and one row per thread");

// The device tables of the three kernels (PoseLayout::fill_kkt_tables).  The words follow pp_word, but the value index is the CCS
// POSITION of the entry in its value run; words behind the last entry are 0.  The three directories are PoseProdTables' own.
struct alignas(16) PoseKktTables {
    int32_t col_word[PP_ENT_CAP];      // CCS position e of jac g: e | its row << PP_IDX_BITS
    int32_t row_word[PP_ENT_CAP];      // position q of the row directory: CCS position of the entry | its column << PP_IDX_BITS
    int32_t touch_word[PP_TOUCH_CAP];  // touch t: CCS position of the Hessian entry | the other variable << PP_IDX_BITS
    int32_t hdiag[PK_WG];              // variable c: CCS position of its diagonal Hessian entry, -1 where the pattern has none (and behind 81)
};

// what a workgroup has staged of one pose: the two value runs by CCS position and the three word tables
struct PoseKktStaged {
    const double* jac;
    const double* hess;
    const int32_t* cw;
    const int32_t* rw;
    const int32_t* tw;
};

// ---- the operator: vec is the vector record [v | w] ------------------------------------------------------------------------------------
HD double pose_kkt_top(const PoseKktStaged& s, int32_t var_dir, int32_t col_dir, const double* vec, bool with_dx, double dx_c, double v_c) {
    const double hv = pose_hv_row(var_dir, s.tw, vec, s.hess);
    const double jt = pose_xbar_column(0.0, 0.0, col_dir, s.cw, vec + PK_BOT, s.jac);
    return kkt_top(with_dx, dx_c, v_c, hv, jt);
}
HD double pose_kkt_bottom(const PoseKktStaged& s, int32_t row_dir, const double* vec, bool with_dc, double dc_i, double w_i) {
    return kkt_bottom(with_dc, dc_i, w_i, pose_jv_row(row_dir, s.rw, vec, s.jac));
}

// ---- the diagonal ----------------------------------------------------------------------------------------------------------------------
// h_cc: the stored diagonal entry of variable c, +0.0 where hdiag is -1
HD double pose_kkt_minv_top(bool with_dx, double h_cc, double dx_c, double floor) { return precond_top(with_dx, h_cc, dx_c, floor); }
// mt: minv_top by pose variable.  The row sum runs from +0.0 in row-table order, q = J * J rounded, d_c last.
HD double pose_kkt_minv_bottom(const PoseKktStaged& s, int32_t row_dir, const double* mt, bool with_dc, double dc_i, double floor) {
    const double sum = precond_row(pp_beg(row_dir), pp_end(row_dir), [&](int e) { return s.jac[s.rw[e] & PP_IDX_MASK]; }, [&](int e) { return mt[s.rw[e] >> PP_IDX_BITS]; });
    return precond_bottom(with_dc, dc_i, sum, floor);
}

// ---- the solve: one element (of the top or of the bottom) of a thread, and the steps of knot_minres.h on it ---------------------------
// A thread without that element keeps zeros: they change no sum and are never stored.
struct PoseKktElem { double y, r1, r2, w, w2, z, v, minv; };

// r1 = r2 = b;  y = M^-1 r2;  w = w2 = z = 0
HD void pose_kkt_elem_start(PoseKktElem& e, double b, bool with_minv, double minv) {
    e.r1 = e.r2 = b;
    e.minv = minv;
    e.y = minres_precond(with_minv, minv, b);
    e.w = e.w2 = e.z = e.v = 0.0;
}
// the per-thread chain of a dot product
HD double pose_kkt_chain(bool has_top, double a_top, double b_top, bool has_row, double a_row, double b_row) {
    double acc = 0.0;
    if (has_top) acc = fm_fma(a_top, b_top, acc);
    if (has_row) acc = fm_fma(a_row, b_row, acc);
    return acc;
}
// v = y / beta
HD void pose_kkt_elem_v(PoseKktElem& e, double beta) { e.v = minres_div(e.y, beta); }
// y = (K v)_e - (beta / oldb) r1 from the second iteration on
HD void pose_kkt_elem_apply(PoseKktElem& e, bool sub, double c1, double kv) { e.y = minres_sub_r1(sub, c1, e.r1, kv); }
// r2_new = y - (alfa / beta) r2;  r1 = r2;  y = M^-1 r2_new
HD void pose_kkt_elem_residual(PoseKktElem& e, double c2, bool with_minv) {
    const double r = minres_new_r2(c2, e.r2, e.y);
    e.r1 = e.r2;
    e.r2 = r;
    e.y = minres_precond(with_minv, e.minv, r);
}
// w_new = (v - oldeps w2 - delta w) / gamma;  z += phi w_new
HD void pose_kkt_elem_update(PoseKktElem& e, const MinresStep& st) {
    const double wn = minres_new_w(st, e.v, e.w2, e.w);
    e.w2 = e.w;
    e.w = wn;
    e.z = minres_new_z(st, wn, e.z);
}

}  // namespace hipnlp
