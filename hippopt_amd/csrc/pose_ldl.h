// pose_ldl.h — a dense L D L^T factorisation of the KKT matrix of ONE pose, with its inertia, a regularisation ladder and the solves
// (hipnlp_pose.hip hipnlp_pose_saddle_ldl_kernel, hipnlp_pose_saddle_ldl_solve_kernel; the test-only CPU emulation tests/pose_ldl_emu runs
// the same text in another order):
//
//     K = [ H + diag d_x + delta I    J^T       ]   order N = 81 + m <= 176, held as a PACKED LOWER triangle, column major:
//         [ J                        -diag d_c  ]   (i, j), i >= j, at pl_at(N, i, j) — 15 576 doubles at most, one workgroup's LDS
//
// H and J are the value runs of pose_kkt.h; PoseLdlTables has the packed place of every stored entry.
//
// ASSEMBLY: every word +0.0, then every stored entry placed once (no pattern has an entry twice: no sums), then the diagonal:
// pl_diag_top (H_cc + d_x,c rounded once, then + delta where a regularisation is active) and pl_diag_bottom (-d_c,i).
//
// FACTORISATION: Bunch-Kaufman partial pivoting, the algorithm of LAPACK's unblocked DSPTF2('L'), alpha = (1 + sqrt 17) / 8, pivots
// 1x1 and 2x2, the pivot vector in LAPACK's convention (1-based; ipiv[k] = kp > 0: a 1x1 pivot, rows and columns k and kp interchanged;
// ipiv[k] = ipiv[k+1] = -kp: a 2x2 pivot, k+1 and kp interchanged).  What could depend on who computes it is pinned:
//   a search (PlMax) returns the largest |a| and among equals the lowest index — pl_max_join is associative and commutative; a value
//     that is not finite anywhere in a searched column or row ends the pose with PL_NONFINITE;
//   the multipliers of a column are formed once: 1x1  l_i = x_i / d (pl_l1, correctly rounded), x the column below the pivot;
//     2x2  pl_w_first / pl_w_second of the two columns (LAPACK's WK, WKP1 with fused multiply-adds);
//   the trailing update is per element, ONE chain each:  1x1  a_ij = fma(-x_i, l_j, a_ij)  (x_i = d l_i: the entry BEFORE the scaling,
//     kept, not multiplied back);  2x2  a_ij = fma(-x1_i, w1_j, fma(-x0_i, w0_j, a_ij)) — so any assignment of elements to lanes gives
//     the same bits.
// ONE departure from DSPTF2's storage: an interchange of step k is ALSO applied to rows kk and kp of the columns in front of the pivot
// block, so that what is stored is the L of  P K P^T = L D L^T  with every interchange applied (the values of DSPTF2's L, D and pivot
// vector; the rows of L in their final places).  That is what lets both triangular solves run in column (axpy) form.
//
// INERTIA is read off D: a 1x1 pivot counts by its sign, a 2x2 block one positive and one negative (Bunch-Kaufman's 2x2 blocks have a
// negative determinant: pl_block_det_negative, asserted by the emulation).  A pivot column that is exactly zero counts as ONE zero, gives
// PL_SINGULAR and ends the factorisation (the pivot vector behind it names every index itself).
//
// SOLVE: b~ = P b (all interchanges, in order); forward  y_i = fma(-L_ik, y_k, y_i)  for every column k ascending; the diagonal (pl_diag1,
// pl_diag2_first / pl_diag2_second: DSPTRS's expressions); backward  y_k = fma(-L_ik, y_i, y_k)  for every row i DESCENDING; x = P^T y.
// Each element takes one fused multiply-add per column, in that order: the bits do not depend on the mapping.  A pose that is not
// PL_OK / PL_EXHAUSTED gets solutions of NaN (pl_nan).
//
// LADDER (IPOPT's inertia correction, top block only): try 0 has delta = 0; try t >= 1 has delta_t, delta_1 = delta_init, delta_(t+1) =
// delta_t * kappa (one rounded product per try), added to all 81 diagonal elements of the top block on a re-assembly from the value runs.
// The ladder ends at the first try with inertia (81, m, 0), at a try that is PL_NONFINITE, or at try max_tries.  The status is that of
// the last try: PL_NONFINITE, PL_SINGULAR, else PL_EXHAUSTED where max_tries > 0 and the inertia is still not (81, m, 0), else PL_OK.
// max_tries = 0: factor once and report whatever the inertia is.
#pragma once
#include <cstdint>

#include "knot_minres.h"
#include "pose_kkt.h"

namespace hipnlp {

constexpr int PL_MAX_N = 176;                                  // 81 + 95: the largest order a workgroup holds
constexpr int PL_MAX_DOUBLES = PL_MAX_N * (PL_MAX_N + 1) / 2;  // 15 576
constexpr int PL_MAX_NRHS = 8;
constexpr int PL_MAX_TRIES = 16;
constexpr double PL_ALPHA = 0.6403882032022076;                // (1 + sqrt 17) / 8
enum { PL_OK = 0, PL_SINGULAR = 1, PL_NONFINITE = 2, PL_EXHAUSTED = 3 };
enum { PL_ONE = 0, PL_FIRST = 1, PL_SECOND = 2 };              // what an index is in D: a 1x1 pivot, the first or the second of a 2x2 block

// the packed lower triangle, column major
HD int pl_col(int N, int j) { return j * N - (j * (j - 1)) / 2; }      // where column j starts (its diagonal element)
HD int pl_at(int N, int i, int j) { return pl_col(N, j) + (i - j); }   // i >= j
HD int pl_doubles(int N) { return (N * (N + 1)) / 2; }

// The device table of the assembly (PoseLayout::fill_ldl_tables): the packed place of every stored entry, by CCS position; -1 behind
// the last entry.  A block of its own beside PoseKktTables.
struct alignas(16) PoseLdlTables {
    int32_t hess_at[PK_HESS_CAP];   // entry (r, c) of the Hessian's lower triangle: pl_at(N, r, c)
    int32_t jac_at[PP_ENT_CAP];     // entry (i, c) of jac g: pl_at(N, 81 + i, c)
};

HD double pl_nan() { return __builtin_nan(""); }
HD double pl_abs(double a) { return __builtin_fabs(a); }

// ---- assembly ----------------------------------------------------------------------------------------------------------------------------
HD double pl_diag_top(double h_cc, bool with_dx, double dx_c, bool with_delta, double delta) {
    const double d = with_dx ? h_cc + dx_c : h_cc;
    return with_delta ? d + delta : d;
}
HD double pl_diag_bottom(bool with_dc, double dc_i) { return with_dc ? -dc_i : 0.0; }
// delta of the next try
HD double pl_next_delta(int next_try, double delta, double delta_init, double kappa) { return next_try == 1 ? delta_init : delta * kappa; }

// ---- the searches ------------------------------------------------------------------------------------------------------------------------
struct PlMax {
    double v;      // the largest |a| among the finite values seen, -1.0: none yet
    int32_t at;    // the lowest index with that |a|
    int32_t bad;   // a value that is not finite was seen
};
HD PlMax pl_max_none() { return PlMax{-1.0, 0x7fffffff, 0}; }
HD PlMax pl_max_of(double a, int at) {
    const bool fin = minres_finite(a);
    return PlMax{fin ? pl_abs(a) : -1.0, fin ? at : 0x7fffffff, fin ? 0 : 1};
}
HD PlMax pl_max_join(PlMax a, PlMax b) {
    const double av = a.v, bv = b.v;          // (the members by value first: nothing is selected by address)
    const int32_t aat = a.at, bat = b.at;
    const bool first = av > bv || (av == bv && aat < bat);
    return PlMax{first ? av : bv, first ? aat : bat, a.bad | b.bad};
}

// ---- the choice of the pivot (DSPTF2) ----------------------------------------------------------------------------------------------------
// absakk = |a_kk|, colmax = the largest |a_ik| below it (0 where there is none)
HD bool pl_column_is_zero(double absakk, double colmax) { return (absakk > colmax ? absakk : colmax) == 0.0; }
HD bool pl_keep_diagonal(double absakk, double colmax) { return absakk >= PL_ALPHA * colmax; }
struct PlPivot { int32_t kp, kstep; };
// rowmax: the largest off-diagonal |a| of row / column imax within the trailing matrix (>= colmax > 0); abs_rr = |a_imax,imax|
HD PlPivot pl_choose(int k, int imax, double absakk, double colmax, double rowmax, double abs_rr) {
    if (absakk >= PL_ALPHA * colmax * minres_div(colmax, rowmax)) return PlPivot{k, 1};
    if (abs_rr >= PL_ALPHA * rowmax) return PlPivot{imax, 1};
    return PlPivot{imax, 2};
}

// ---- the multipliers and the trailing update ---------------------------------------------------------------------------------------------
HD double pl_l1(double x_i, double d) { return minres_div(x_i, d); }
HD double pl_update1(double a_ij, double x_i, double l_j) { return fm_fma(-x_i, l_j, a_ij); }
// a 2x2 block [a_kk a_21; a_21 a_11] scaled as DSPTF2 scales it
struct PlBlock { double d11, d22, d21, det; };
HD PlBlock pl_block(double a_kk, double a_21, double a_11) {
    PlBlock b;
    b.d11 = minres_div(a_11, a_21);
    b.d22 = minres_div(a_kk, a_21);
    b.det = fm_fma(b.d11, b.d22, -1.0);                   // (a_kk a_11 - a_21^2) / a_21^2
    b.d21 = minres_div(minres_div(1.0, b.det), a_21);
    return b;
}
HD bool pl_block_det_negative(const PlBlock& b) { return b.det < 0.0; }
HD double pl_w_first(const PlBlock& b, double x0_j, double x1_j) { return b.d21 * fm_fma(b.d11, x0_j, -x1_j); }
HD double pl_w_second(const PlBlock& b, double x0_j, double x1_j) { return b.d21 * fm_fma(b.d22, x1_j, -x0_j); }
HD double pl_update2(double a_ij, double x0_i, double x1_i, double w0_j, double w1_j) { return fm_fma(-x1_i, w1_j, fm_fma(-x0_i, w0_j, a_ij)); }

// ---- the solve ---------------------------------------------------------------------------------------------------------------------------
HD double pl_axpy(double y_i, double l, double y_k) { return fm_fma(-l, y_k, y_i); }
HD double pl_diag1(double y, double d) { return minres_div(y, d); }
struct PlSolveBlock { double akm1, ak, denom, a21; };
HD PlSolveBlock pl_solve_block(double a_kk, double a_21, double a_11) {
    PlSolveBlock b;
    b.a21 = a_21;
    b.akm1 = minres_div(a_kk, a_21);
    b.ak = minres_div(a_11, a_21);
    b.denom = fm_fma(b.akm1, b.ak, -1.0);
    return b;
}
HD double pl_diag2_first(const PlSolveBlock& b, double y_k, double y_k1) {
    return minres_div(fm_fma(b.ak, minres_div(y_k, b.a21), -minres_div(y_k1, b.a21)), b.denom);
}
HD double pl_diag2_second(const PlSolveBlock& b, double y_k, double y_k1) {
    return minres_div(fm_fma(b.akm1, minres_div(y_k1, b.a21), -minres_div(y_k, b.a21)), b.denom);
}

// ---- the ladder --------------------------------------------------------------------------------------------------------------------------
HD bool pl_inertia_wanted(int pos, int neg, int zero, int m) { return pos == POSE_NX && neg == m && zero == 0; }
HD bool pl_ladder_goes_on(int status, bool wanted, int t, int max_tries) { return status != PL_NONFINITE && !wanted && t < max_tries; }
HD int pl_final_status(int status, bool wanted, int max_tries) { return status != PL_OK ? status : ((max_tries > 0 && !wanted) ? PL_EXHAUSTED : PL_OK); }

// ---- what the two entry points refuse before anything is launched (nullptr: nothing) ------------------------------------------------------
inline const char* pl_solve_call_error(bool factor, bool pivots, int nrhs, bool rhs_top, bool rhs_bottom, bool sol_top, bool sol_bottom) {
    if (!factor || !pivots) return "factor_dev and pivots_dev are required";
    if (nrhs < 1 || nrhs > PL_MAX_NRHS) return "1 <= nrhs <= 8";
    if (!rhs_top || !rhs_bottom || !sol_top || !sol_bottom) return "a right-hand side or solution pointer is null";
    return nullptr;
}
inline const char* pl_factor_call_error(bool hess, bool jac, int nrhs, bool rhs_top, bool rhs_bottom, bool sol_top, bool sol_bottom, bool inertia, bool status, double delta_init,
                                        double kappa, int max_tries, bool factor, bool pivots) {
    if (!hess || !jac || !inertia || !status) return "hess_values_dev, jac_values_dev, inertia_dev and status_dev are required";
    if (nrhs < 0 || nrhs > PL_MAX_NRHS) return "0 <= nrhs <= 8";
    if (nrhs > 0 && (!rhs_top || !rhs_bottom || !sol_top || !sol_bottom)) return "a right-hand side or solution pointer is null with nrhs > 0";
    if (factor != pivots) return "factor_dev and pivots_dev: both or neither";
    if (max_tries < 0 || max_tries > PL_MAX_TRIES) return "0 <= max_tries <= 16";
    if (max_tries > 0 && (!minres_finite(delta_init) || !(delta_init > 0.0))) return "delta_init must be a finite number > 0 with max_tries > 0";
    if (max_tries > 0 && (!minres_finite(kappa) || !(kappa > 1.0))) return "kappa must be a finite number > 1 with max_tries > 0";
    return nullptr;
}

}  // namespace hipnlp
