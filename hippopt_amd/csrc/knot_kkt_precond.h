// knot_kkt_precond.h — the diagonal preconditioner M^-1 = diag(minv_top, minv_bottom) > 0 of the MINRES solve of knot_minres.h, built from the
// STORED value runs of the KKT operator of knot_kkt.h (hipnlp.hip hipnlp_kkt_diag_precond_device / hipnlp_saddle_diag_kernel; the test-only
// CPU emulation tests/kkt_precond_emu runs the same text):
//
//     a_j        = | H_jj + d_x,j |                        H_jj: the stored diagonal entry of variable j, +0.0 where the pattern has none (the six
//                                                          horizon-global variables); without d_x: | H_jj |
//     minv_top_j = 1 / max(a_j, floor)
//     s_i        = d_c,i + sum_e J_ie^2 minv_top_col(e)    the entries of row i in the order of JprodTables (ascending global column); without
//                                                          d_c: no first term
//     minv_bot_i = 1 / max(| s_i |, floor)
//
// The absolute value on the top is deliberate: H + diag d_x is indefinite at real iterates and MINRES needs M positive definite.  The bottom
// is the diagonal of the Schur complement d_c + J M_top^-1 J^T of the block-diagonal stand-in for K.
//
// The rounding sequence, on both sides:
//   top     t = H_jj + d_x,j (one rounded add; t = H_jj without d_x);  a = |t|;  d = a < floor ? floor : a;  r = 1 / d correctly rounded
//           (minres_div);  the result is r — unless a is not finite (a - a != 0: a NaN or an infinity of the inputs), then it is the NaN a - a:
//           the comparison with the floor lets a NaN through, and this keeps 1 / inf = 0 from hiding an infinity.  MINRES ends such a
//           trajectory with status 2.
//   bottom  ONE chain per row from acc = +0.0 over its entries in table order:  q = J_ie * J_ie (one rounded multiply);
//           acc = fma(q, minv_top_col(e), acc);  then s = acc + d_c,i (one rounded add, LAST; s = acc without d_c);  then as the top with
//           t = s.
// minv_top of a neighbouring knot's variables (the predecessor's, the other horizon end's, the globals) is RECOMPUTED by every workgroup
// that needs it, not communicated: the same expression on the same inputs, so the same bits.  No workgroup waits for another, there are no
// atomics, and every sum has a fixed order.
//
// Who writes what is minres_owned (knot_minres.h): every element of both outputs is written exactly once, by the workgroup that writes that
// element of K v.
#pragma once
#include "knot_jprod.h"
#include "knot_minres.h"

namespace hipnlp {

// 1 / max(|t|, floor), a non-finite t passed on as NaN
HD double precond_reciprocal(double t, double floor) {
    const double a = t < 0.0 ? -t : t;   // (a NaN stays)
    const double d = a < floor ? floor : a;
    const double r = minres_div(1.0, d);
    const double bad = a - a;            // +0.0 for a finite a, NaN otherwise
    return bad == 0.0 ? r : bad;
}

// minv_top_j from the stored diagonal entry (+0.0: none) and d_x,j
HD double precond_top(bool with_dx, double h_jj, double dx_j, double floor) { return precond_reciprocal(with_dx ? h_jj + dx_j : h_jj, floor); }

// sum_e J_ie^2 minv_top_col(e) over the entries [beg, end) of an owned row: val(e) / mt(e) the value of entry e and minv_top of its column,
// wherever the caller keeps them
template <class Val, class Mt> HD double precond_row(int beg, int end, const Val& val, const Mt& mt) {
    double acc = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
    for (int e = beg; e < end; ++e) {
        const double jv = val(e);
        const double q = jv * jv;
        acc = fm_fma(q, mt(e), acc);
    }
    return acc;
}
// ... from the staged words w, values jv and the records ms of minv_top in the JP_V_* arrangement (what jprod_row_staged reads for v)
HD double precond_row_staged(int32_t dir, const int32_t* w, const double* jv, const double* ms) {
    const int beg = dir & JP_POS_MASK, end = beg + (dir >> JP_POS_BITS);
    return precond_row(beg, end, [&](int e) { return jv[w[e] & JP_POS_MASK]; }, [&](int e) { return ms[w[e] >> JP_POS_BITS]; });
}

// minv_bottom_i from the finished row sum and d_c,i
HD double precond_bottom(bool with_dc, double dc_i, double row_sum, double floor) { return precond_reciprocal(with_dc ? row_sum + dc_i : row_sum, floor); }

}  // namespace hipnlp
