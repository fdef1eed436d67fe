// knot_ldl.h — the block top of a preconditioner for the MINRES solve of knot_minres.h: a dense L D L^T of every knot's block of
// H + diag d_x, with its inertia, and M_k^-1 = P^T L^-T |D|^-1 L^-1 P applied from the stored factor (hipnlp.hip
// hipnlp_kkt_block_factor_kernel, hipnlp_kkt_block_apply_kernel, hipnlp_kkt_minres_block_first_kernel; the test-only CPU emulation
// tests/kkt_block_emu runs the same text in another element order):
//
//     M^-1 = blockdiag_k( P_k^T L_k^-T |D_k|^-1 L_k^-1 P_k )  (+)  diag(minv_top of the six globals)  (+)  diag(minv_bottom)
//
// The Hessian of the Lagrangian is block diagonal by knot (knot_hess_layout.h): block k has order NXK = 189 and is held as a PACKED LOWER
// triangle, column major, (i, j) at pl_at(189, i, j) — 17 955 doubles, 143 640 B of one workgroup's LDS.  The periodicity coupling of the
// two horizon ends, where a pattern has it, is NOT part of any block: M stays block diagonal (and positive definite) without it.  The
// globals' and the bottom's diagonal are those of knot_kkt_precond.h, from its own launch.  The element-level expressions, the searches'
// join and the choice of the pivot are pose_ldl.h's at order 189; what follows is what differs or is new.
//
// ASSEMBLY: every word +0.0, then every stored entry of the knot's block placed once through KnotLdlTables (no entry occurs twice: no
// sums), then the diagonal: H_cc + d_x,c rounded once (pl_diag_top without a regularisation); without d_x: H_cc.
//
// FACTORISATION: pose_ldl.h's — DSPTF2('L') pivoting, ties to the lowest index, one fused multiply-add chain per element, interchanges
// also applied in front of the pivot block — with ONE difference: a pivot column that is exactly zero does NOT end the factorisation.
// Nothing is interchanged or updated, its L column stays the zeros it is, it counts as ONE zero of the inertia, and the step is a 1x1
// step.  A value that is not finite in a searched column or row gives the knot KL_NONFINITE: its stored factor, e and o are then the
// NaN of pl_nan() in every word, its pivot words name every index itself, its inertia is (0, 0, 0).
//
// THE PIVOT WORD of index i (int32): bits 0..15 LAPACK's ipiv[i] as a 16-bit two's complement (pose_ldl.h's convention), bits 16..23
// perm[i] (b~_i = b_perm[i] after every interchange), bits 24..25 what i is in D (PL_ONE / PL_FIRST / PL_SECOND) — so that applying the
// factor needs no serial walk over the pivot vector.
//
// |D|^-1 is stored as two vectors: e [189] its diagonal and o [189] the coupling of index i to i + 1, +0.0 where i is not the first
// index of a 2x2 block.  floor > 0:
//   1x1  e = 1 / max(|d|, floor)                                                                    (kl_floored_inverse)
//   2x2  D = [a b; b c] = m I + r R,  m = (a + c)/2,  h = (a - c)/2,  r = sqrt(h^2 + b^2),  R = [ch sh; sh -ch],  ch = h/r,  sh = b/r;
//        its eigenvalues are m + r and m - r with the projectors (I + R)/2 and (I - R)/2, so with mu_1 = 1 / max(|m + r|, floor),
//        mu_2 = 1 / max(|m - r|, floor):  |D|^-1 = lo I + span (I + sg R)/2,  lo = min(mu), span = |mu_1 - mu_2|, sg = +1 where
//        mu_1 >= mu_2, else -1.  Every element is one fused multiply-add onto lo > 0 of a product that is >= 0 (|ch| <= 1: the
//        correctly rounded sqrt(fma(h, h, b b)) is >= |h|), so e > 0 always; e_k e_(k+1) > o_k^2 holds while span^2 u < mu_1 mu_2,
//        i.e. cond(|D_block|) below about 1e15 — the emulation asserts it for every block it forms.          (kl_abs_inverse2)
// D itself stays in the stored factor.
//
// APPLY  z = P^T L^-T |D|^-1 L^-1 P r:  y_i = r_perm[i];  forward  y_i = fma(-L_ik, y_k, y_i)  for every column k ASCENDING (the element
// (k + 1, k) of a 2x2 block is D's, not L's: skipped);  the diagonal, every element from the y of before it:
// t_i = fma(o_(i-1), y_(i-1), fma(o_i, y_(i+1), e_i y_i))  with o_(-1) = y_(-1) = y_189 = +0.0  (kl_diag3);  backward
// t_k = fma(-L_ik, t_i, t_k)  for every row i DESCENDING;  z_perm[i] = t_i.  Each element takes one fused multiply-add per column, in
// that order: the bits do not depend on the mapping.  A knot whose e_0 is NaN (KL_NONFINITE) yields pl_nan() for its 189 elements.
//
// LADDER (hipnlp_kkt_block_ladder_kernel; the test-only CPU emulation tests/kkt_ladder_emu): pose_ldl.h's inertia-correction ladder, climbed
// by every knot on its own, inside the launch that holds its block.  Try 0 has delta = 0 and is the ASSEMBLY above, bit for bit.  Try
// t >= 1 has delta_t = pl_next_delta(t, delta_(t-1), delta_init, kappa) — delta_1 = delta_init, then one rounded product per try — and is
// a FULL re-assembly from the Hessian run in memory: every word +0.0, every stored entry through KnotLdlTables, then the diagonal
// pl_diag_top(h, with_dx, dx_c, true, delta_t) = (H_cc + d_x,c) + delta_t, two roundings in that order.  Every try is a whole
// factorisation (no exit at the first pivot that is not positive), so the inertia reported for a knot is complete whatever its status.
// The ladder ends at the first try whose inertia is (189, 0, 0) (kl_inertia_wanted), at a try that is KL_NONFINITE, or at try max_tries;
// factor, pivot words, e, o, inertia, delta and tries are the LAST try's.  Status (kl_ladder_final_status): KL_NONFINITE, else
// KL_EXHAUSTED where max_tries > 0 and the inertia is still not wanted, else KL_OK.  There is no status 1: a zero pivot column counts as
// one zero and the factorisation goes on — the inertia is then not wanted and the ladder climbs.  max_tries = 0: one factorisation, the
// bits of the factor kernel, status KL_OK whatever the inertia.
// WHAT A KL_OK OF A LADDER WITH max_tries > 0 MEANS: every pivot of the stored factor is 1x1 and positive (a Bunch-Kaufman 2x2 block has
// a negative determinant, so it would have counted one negative), so |D| = D where no |d| is below the floor, o = 0, and APPLY from this
// record is the inverse of H_k + diag d_x,k + delta_k I, not of an absolute value of it.  With every knot KL_OK, the six globals' d_x > 0
// and d_c > 0, K' = [[A, J^T], [J, -diag d_c]] with A = blockdiag_k(H_k + d_x,k + delta_k I) (+) diag(d_x of the globals) is symmetric
// quasi-definite: its inertia is (n, m, 0) without anybody factoring K'.  SUFFICIENT, NOT NECESSARY: IPOPT needs only the Hessian reduced
// to the null space of J positive definite and perturbs with ONE delta for the whole matrix; a delta per knot on the whole block can be
// larger than that needs, and is never smaller than what the block alone needs at the ladder's resolution (a factor kappa).
#pragma once
#include <cstdint>

#include "knot_hess_body.h"
#include "knot_kkt_precond.h"
#include "knot_minres.h"
#include "pose_ldl.h"

namespace hipnlp {

constexpr int KL_N = NXK;                                // 189: the order of a knot's block
constexpr int KL_DOUBLES = KL_N * (KL_N + 1) / 2;        // 17 955
constexpr int KL_ENT_CAP = (hk::COUNT + 255) / 256 * 256;   // entries of a knot's block of the Hessian run, at most
enum { KL_OK = 0, KL_NONFINITE = 2, KL_EXHAUSTED = 3 };   // (no 1: a zero pivot column does not end a knot's factorisation)
static_assert(KL_DOUBLES * int(sizeof(double)) == 143640 && KL_N <= 3 * 64 && KL_N < 256, "a packed block in one workgroup's LDS; three elements per lane; perm in eight bits");

// The device table of the assembly (HessLayout::fill_ldl_tables): the packed place of the entry at every position of a knot's block, -1
// behind the last entry.  A block of its own beside HvpTables.
struct alignas(16) KnotLdlTables {
    int32_t at[KL_ENT_CAP];
};

// ---- the pivot word ----------------------------------------------------------------------------------------------------------------------
HD int32_t kl_word(int ipiv, int perm, int kind) { return int32_t((uint32_t(ipiv) & 0xffffu) | (uint32_t(perm) << 16) | (uint32_t(kind) << 24)); }
HD int kl_word_ipiv(int32_t w) { return int(int16_t(uint16_t(uint32_t(w) & 0xffffu))); }
HD int kl_word_perm(int32_t w) { return int((uint32_t(w) >> 16) & 0xffu); }
HD int kl_word_kind(int32_t w) { return int((uint32_t(w) >> 24) & 3u); }

// ---- |D|^-1 ------------------------------------------------------------------------------------------------------------------------------
HD double kl_floored_inverse(double lambda, double floor) {
    const double a = pl_abs(lambda);
    return minres_div(1.0, a < floor ? floor : a);
}
struct KlAbsInv2 { double e0, e1, o; };
// the block [a b; b c] of D as the factor stores it: a at the diagonal of column k, b below it, c at the diagonal of column k + 1
HD KlAbsInv2 kl_abs_inverse2(double a, double b, double c, double floor) {
    const double h = 0.5 * (a - c), m = 0.5 * (a + c);
    const double r = minres_sqrt(fm_fma(h, h, b * b));
    const double mu1 = kl_floored_inverse(m + r, floor), mu2 = kl_floored_inverse(m - r, floor);
    const double ch = minres_div(h, r), sh = minres_div(b, r);
    const bool first = mu1 >= mu2;
    const double lo = first ? mu2 : mu1, span = first ? mu1 - mu2 : mu2 - mu1, sg = first ? 1.0 : -1.0;
    KlAbsInv2 q;
    q.e0 = fm_fma(span, 0.5 * fm_fma(sg, ch, 1.0), lo);
    q.e1 = fm_fma(span, 0.5 * fm_fma(-sg, ch, 1.0), lo);
    q.o = span * (0.5 * (sg * sh));
    return q;
}
HD bool kl_block_positive_definite(double e0, double e1, double o) { return e0 > 0.0 && e1 > 0.0 && e0 * e1 > o * o; }

// the diagonal of the apply at index i: y_dn = y_(i-1), y_up = y_(i+1), o_dn = o_(i-1); +0.0 for what lies outside 0 .. 188
HD double kl_diag3(double e_i, double y_i, double o_i, double y_up, double o_dn, double y_dn) { return fm_fma(o_dn, y_dn, fm_fma(o_i, y_up, e_i * y_i)); }

// whether the knot's stored e says that it can be applied (KL_NONFINITE stores NaN in every word)
HD bool kl_good(double e_first) { return e_first == e_first; }

// ---- the ladder (the delta of a try: pl_next_delta; whether another try follows: pl_ladder_goes_on) --------------------------------------------
HD bool kl_inertia_wanted(int pos, int neg, int zero) { return pos == KL_N && neg == 0 && zero == 0; }
HD int kl_ladder_final_status(int status, bool wanted, int max_tries) { return status != KL_OK ? status : ((max_tries > 0 && !wanted) ? KL_EXHAUSTED : KL_OK); }
static_assert(KL_NONFINITE == PL_NONFINITE && KL_EXHAUSTED == PL_EXHAUSTED && KL_OK == PL_OK, "pl_ladder_goes_on reads a knot's status");

// ---- what the entry points refuse before anything is launched (nullptr: nothing) ------------------------------------------------------------
inline const char* kl_factor_call_error(bool hess, double floor, bool factor, bool pivots, bool e, bool o, bool inertia, bool status) {
    if (!hess) return "hess_values_dev is required";
    if (!factor || !pivots || !e || !o) return "factor_dev, pivots_dev, e_dev and o_dev are required";
    if (!inertia || !status) return "inertia_dev and status_dev are required";
    if (!(floor > 0.0) || !minres_finite(floor)) return "floor must be a finite number > 0";
    return nullptr;
}
// the ladder's entry point: the factor entry point's refusals, then its own (pl_factor_call_error's for the three ladder arguments)
inline const char* kl_ladder_call_error(bool hess, double floor, double delta_init, double kappa, int max_tries, bool factor, bool pivots, bool e, bool o, bool inertia, bool status,
                                        bool delta, bool tries) {
    if (const char* r = kl_factor_call_error(hess, floor, factor, pivots, e, o, inertia, status)) return r;
    if (!delta || !tries) return "delta_dev and tries_dev are required";
    if (max_tries < 0 || max_tries > PL_MAX_TRIES) return "0 <= max_tries <= 16";
    if (max_tries > 0 && (!minres_finite(delta_init) || !(delta_init > 0.0))) return "delta_init must be a finite number > 0 with max_tries > 0";
    if (max_tries > 0 && (!minres_finite(kappa) || !(kappa > 1.0))) return "kappa must be a finite number > 1 with max_tries > 0";
    return nullptr;
}
inline const char* kl_apply_call_error(bool factor, bool pivots, bool e, bool o, bool minv_top, bool minv_bottom, bool r_top, bool r_bottom, bool z_top, bool z_bottom) {
    if (!factor || !pivots || !e || !o) return "factor_dev, pivots_dev, e_dev and o_dev are required";
    if (!minv_top || !minv_bottom) return "minv_top_dev and minv_bottom_dev are required";
    if (!r_top || !r_bottom || !z_top || !z_bottom) return "a vector pointer is null";
    return nullptr;
}
inline const char* kl_minres_call_error(bool hess, bool jac, bool factor, bool pivots, bool e, bool o, bool minv_top, bool minv_bottom, bool rhs_top, bool rhs_bottom,
                                        bool sol_top, bool sol_bottom, bool iterations, bool residual, bool status, double rtol, int max_iterations, int check_every) {
    if (!hess || !jac) return "hess_values_dev and jac_values_dev are required";
    if (!factor || !pivots || !e || !o) return "factor_dev, pivots_dev, e_dev and o_dev are required";
    if (!minv_top || !minv_bottom) return "minv_top_dev and minv_bottom_dev are required";
    if (!rhs_top || !rhs_bottom || !sol_top || !sol_bottom) return "a right-hand side or solution pointer is null";
    if (!iterations || !residual || !status) return "iterations_dev, residual_dev and status_dev are required";
    if (!(rtol >= 0.0)) return "rtol >= 0";
    if (max_iterations < 0) return "max_iterations >= 0";
    if (check_every < 0) return "check_every >= 0";
    return nullptr;
}

}  // namespace hipnlp
