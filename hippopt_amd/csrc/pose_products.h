// pose_products.h — the three products of the static pose finder NLP that one workgroup sums from what its program leaves in LDS
// (hipnlp_pose.hip hipnlp_pose_lgrad_kernel, hipnlp_pose_jvp_kernel, hipnlp_pose_hvp_kernel; the test-only CPU emulation runs the same code):
//   xbar = sigma grad f(x) + J(x)^T lambda      one thread per column, over the column's entries in CCS order
//   J(x) v  and  grad f(x) . v                   one thread per row, over the row's entries in ascending column; one lane for the dot product
//   H(x, sigma, lambda) v                        one thread per variable, over the variable's touches of the lower triangle in CCS order
//
// A pose is one workgroup: every entry of jac g is in the cut staging of the pose program (pose_body.h pjs) when it ends, every entry of
// the Hessian of the Lagrangian in HessScratch::H when the Hessian program ends.  No other workgroup contributes to a sum, there are no
// atomics, and the order of every sum is the order of a table PoseLayout::build writes — the same bits on every launch.
#pragma once
#include <cstdint>

#include "knot_hvp.h"
#include "knot_lgrad.h"
#include "pose_hess_body.h"

namespace hipnlp {

// What the device kernels stage per workgroup of 256 threads, and PoseLayout::build checks a handle's tables against:
//   entries of jac g: four words per thread (the copy-out of hipnlp_pose_kernel holds as many);
//   rows of g: one per thread (one multiplier staged, one row summed);
//   touches of the Hessian: six words per thread (every entry of the lower triangle touches its row and, off the diagonal, its column).
constexpr int PP_WG = 256;
constexpr int PP_ENT_CAP = 4 * PP_WG;
constexpr int PP_ROW_CAP = PP_WG;
constexpr int PP_TOUCH_CAP = 6 * PP_WG;
// an entry / touch word: the index of the value (Jacobian staging index, native Hessian slot) in bits 0..11, the index of the factor
// (row of the multiplier, column or other variable of v) in bits 12..
// a directory word (one column, row or variable): first entry in bits 0..11, number of entries in bits 12..
constexpr int PP_IDX_BITS = 12, PP_CNT_MAX = 255;
constexpr int32_t PP_IDX_MASK = (1 << PP_IDX_BITS) - 1;
static_assert(js::COUNT <= (1 << PP_IDX_BITS) && hs::COUNT <= (1 << PP_IDX_BITS) && PP_ENT_CAP <= (1 << PP_IDX_BITS) && PP_TOUCH_CAP <= (1 << PP_IDX_BITS), "value index of a word");
static_assert(PP_ROW_CAP < (1 << (31 - PP_IDX_BITS)) && POSE_NX <= PP_WG && 2 * hs::COUNT <= PP_TOUCH_CAP, "factor index of a word; one column / variable per thread");

HD constexpr int32_t pp_word(int value_index, int factor_index) { return int32_t(value_index) | (int32_t(factor_index) << PP_IDX_BITS); }
HD constexpr int pp_beg(int32_t dir) { return dir & PP_IDX_MASK; }
HD constexpr int pp_end(int32_t dir) { return (dir & PP_IDX_MASK) + (dir >> PP_IDX_BITS); }

// The device tables of the three kernels (hipnlp_pose_create fills them from a PoseLayout; words behind the last entry are 0, directory
// words behind the last column / row / variable are 0: an empty range).
struct alignas(16) PoseProdTables {
    int32_t col_word[PP_ENT_CAP];      // CCS position e: staging index of the entry | its row << PP_IDX_BITS
    int32_t row_word[PP_ENT_CAP];      // position q of the row directory: staging index of the entry | its column << PP_IDX_BITS
    int32_t touch_word[PP_TOUCH_CAP];  // touch t: native Hessian slot of the entry | the other variable << PP_IDX_BITS
    int32_t col_dir[PP_WG];            // column c: first CCS position | entries << PP_IDX_BITS
    int32_t row_dir[PP_WG];            // row i: first position of the row directory | entries << PP_IDX_BITS
    int32_t var_dir[PP_WG];            // variable i: first touch | touches << PP_IDX_BITS
};

// xbar_c: sigma grad_c, then lambda_row J_row,c over the column's CCS positions in order (knot_lgrad.h lgrad_column).
// w: the staged col_word, lam: the staged multipliers by row, jac: the pose program's cut Jacobian staging.
HD double pose_xbar_column(double sigma, double grad_c, int32_t dir, const int32_t* w, const double* lam, const double* jac) {
    return lgrad_column(sigma, grad_c, pp_beg(dir), pp_end(dir), [&](int e) { return lam[w[e] >> PP_IDX_BITS]; }, [&](int e) { return jac[w[e] & PP_IDX_MASK]; });
}

// (J v)_i: from +0.0, J_i,c v_c over the row's entries in ascending column (knot_hvp.h hvp_row without a coupling term).
// w: the staged row_word, v: the staged direction by pose variable.
HD double pose_jv_row(int32_t dir, const int32_t* w, const double* v, const double* jac) {
    return hvp_row(pp_beg(dir), pp_end(dir), [&](int e) { return jac[w[e] & PP_IDX_MASK]; }, [&](int e) { return v[w[e] >> PP_IDX_BITS]; }, false, 0.0, 0.0);
}

// grad f . v: from +0.0, the 81 products in the order of the pose's variables, one lane.  grad: the gradient staging of the scratch (by
// column of the knot record), v: by pose variable.
HD double pose_gradf_dot_v(const double* grad, const double* v) {
    double acc = 0.0;
    for (int c = 0; c < POSE_NX; ++c) acc = fm_fma(grad[pose_to_knot_col(c)], v[c], acc);
    return acc;
}

// (H v)_i: from +0.0, H_e v_other over the variable's touches in order (knot_hvp.h hvp_row without a coupling term).
// w: the staged touch_word, H: HessScratch::H.
HD double pose_hv_row(int32_t dir, const int32_t* w, const double* v, const double* H) {
    return hvp_row(pp_beg(dir), pp_end(dir), [&](int e) { return H[w[e] & PP_IDX_MASK]; }, [&](int e) { return v[w[e] >> PP_IDX_BITS]; }, false, 0.0, 0.0);
}

}  // namespace hipnlp
