// knot_kkt.h — one application of the KKT operator of an interior-point step from STORED value runs (hipnlp.hip hipnlp_kkt_times_kernel;
// the test-only CPU emulation runs the same code):
//
//     K(x, sigma, lambda; d_x, d_c) [v; w] = [ (H + diag d_x) v + J^T w ]   top     [n]
//                                            [  J v - diag(d_c) w       ]   bottom  [m]
//
// Nothing is summed here that another header does not already sum: H v is hvp_row (knot_hvp.h) over the touch lists of HessLayout, J^T w
// is jprod_column_staged and J v is jprod_row_staged (knot_jprod.h) over the directories of Layout.  H is block diagonal by knot, the
// columns of jac g are knot-local and every row of g has one owner knot, so one workgroup per (trajectory, knot) holds everything its 189
// elements of `top` and its owned rows of `bottom` need.  This header has only the two expressions that combine the finished sums with
// the diagonals, so that device and emulation round the same way.
#pragma once
#include "knot_hvp.h"
#include "knot_jprod.h"

namespace hipnlp {

// top_c = hv + jt, hv = (H v)_c (+0.0 for a horizon-global variable: no entry of the Hessian touches it), jt = (J^T w)_c: one add, what a
// caller who composes the product from hipnlp_hess_times_device and hipnlp_jac_transpose_times_device gets.  With the diagonal: ONE fused
// multiply-add d_x,c v_c + (hv + jt) on top of that sum.
HD double kkt_top(bool with_dx, double dx_c, double v_c, double hv, double jt) {
    const double s = hv + jt;
    return with_dx ? fm_fma(dx_c, v_c, s) : s;
}
// bottom_i = jv, jv = (J v)_i; with the diagonal: ONE fused multiply-add (-d_c,i) w_i + jv.
HD double kkt_bottom(bool with_dc, double dc_i, double w_i, double jv) { return with_dc ? fm_fma(-dc_i, w_i, jv) : jv; }

}  // namespace hipnlp
