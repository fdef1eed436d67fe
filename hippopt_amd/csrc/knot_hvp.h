// knot_hvp.h — the Hessian-vector product  y = H(x, sigma, lambda) v  of one knot's variables, summed from the entries of the knot's block
// of the Hessian of the Lagrangian (hipnlp.hip hipnlp_knot_hvp_kernel, hipnlp_hess_times_kernel; the test-only CPU emulation runs the
// same code).
//
// The Hessian is block diagonal by knot (knot_hess_layout.h): every entry has its row and its column in the same knot record, so the 189
// variables of knot k are sums over entries one workgroup already holds — no other workgroup contributes, no atomics, and the order of the
// sum is fixed.  An entry of the lower triangle "touches" its row and, off the diagonal, its column; HessLayout::build lists the touches
// of every variable in block-position order.  Only the periodicity as a cost couples two knots: variable i of the last knot with the SAME
// variable of the first one, by a value that does not depend on x — one more term at both ends, added last.
#pragma once
#include <cstdint>

#include "knot_tanh.h"
#include "nlp_defs.h"

namespace hipnlp {

// One touch of a variable: the entry's position in the knot block (value runs in memory), its native slot (the Hessian program's
// staging), and the OTHER variable of the entry (the variable itself on the diagonal).
struct HvpTouch { int32_t pos, slot, other; };

// touch words of a block: fourteen per thread of 256 (the device kernels stage them in LDS); HessLayout::build checks a handle's tables
constexpr int HVP_WORD_CAP = 14 * 256;
// a device touch word: native slot (fused kernel) or block position (stored values) in bits 0..11, the other variable in bits 12..
constexpr int HVP_IDX_BITS = 12;
// a device row word (variable i): first touch in bits 0..11, number of touches in bits 12..19, bit 20: the variable has a coupling term
constexpr int HVP_CNT_BITS = 8, HVP_COUPLED_BIT = HVP_IDX_BITS + HVP_CNT_BITS;
static_assert(HVP_WORD_CAP <= (1 << HVP_IDX_BITS) && NXK < (1 << (31 - HVP_IDX_BITS)), "Hessian-vector touch word");

// y of one variable: the touches [beg, end) in the order of the table, from +0.0, one fused multiply-add each; then, where the variable
// is coupled with the other end of the horizon, c v_other_end.  val(e) / vec(e): the value of touch e's entry and the element of v at
// its other variable, wherever the caller keeps them (neither depends on the running sum: the reads can all be in flight).
template <class Val, class Vec> HD double hvp_row(int beg, int end, const Val& val, const Vec& vec, bool coupled, double c, double v_other_end) {
    double acc = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
    for (int e = beg; e < end; ++e) acc = fm_fma(val(e), vec(e), acc);
    if (coupled) acc = fm_fma(c, v_other_end, acc);
    return acc;
}

}  // namespace hipnlp
