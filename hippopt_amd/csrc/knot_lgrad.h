// knot_lgrad.h — the Lagrangian gradient  xbar = sigma grad f(x) + J(x)^T lambda  of one knot's columns, summed from what the knot
// program leaves in its scratch (hipnlp.hip hipnlp_knot_lgrad_kernel; the test-only CPU emulation runs the same code).
//
// Every entry of jac g whose column belongs to knot k is emitted by knot k's program: the 189 columns of the knot are a sum
// over entries one workgroup already holds — no other workgroup contributes, no atomics, and the order of the sum is fixed.  Layout::build
// lists the entries of a first / interior / last block in (column, row) order whatever the jac order of the handle (CCS or varying first):
// both give the same bits.
#pragma once
#include <cstdint>

#include "knot_body.h"

namespace hipnlp {

// One entry of a knot block of jac g: native slot of the knot program, column within the knot (0 .. NXK-1; horizon-global entries:
// 0 .. NXG-1), row of g at knot k = row_a + row_b k, and the position of that row in the knot's list of multipliers (Layout::lg_rows).
struct LgradEntry { int32_t slot, col, row_a, row_b, lam; };

// Where the multipliers go once the knot program has ended (nothing reads the scratch then but the reduction, which needs grad and jac):
// the g staging of the compact scratch — the program never reads its staged g back — and, in front of it, the union of the joint records,
// own[] and the horizon-end rows (ScratchJrOwn<LAYOUT_COMPACT>: 793 words).  A last knot with both horizon ends as constraints touches 439
// rows, more than the 361 words of the g staging alone.  The kernel holds them in registers across the program: two per thread of 256.
template <class S> HD double* lgrad_lam_stage(S& s) { return &s.Jr[0].d[0]; }
constexpr int LG_LAM_CAP = 2 * 256;
static_assert(LG_LAM_CAP * sizeof(double) <= sizeof(ScratchJrOwn<LAYOUT_COMPACT>), "multiplier staging");
// entry words of a block: seven per thread of 256 (hipnlp.hip stages them in arrays of the scratch that are dead once the program has
// ended); Layout::build checks a handle's tables against both capacities
constexpr int LG_ENT_CAP = 7 * 256;
// a device entry word: native slot in bits 0..11, the position of the entry's multiplier in bits 12..
constexpr int LG_SLOT_BITS = 12;
static_assert(js::COUNT <= (1 << LG_SLOT_BITS) && LG_LAM_CAP < (1 << (31 - LG_SLOT_BITS)), "lgrad entry word");

// xbar of one column: sigma grad_c first, then lambda_row J_row,c of the entries [beg, end) in the order of the table — one fused
// multiply-add each.  lam(e) / jac(e): the multiplier of entry e's row and the entry's value, wherever the caller keeps them.
template <class Lam, class Jac> HD double lgrad_column(double sigma, double grad_c, int beg, int end, const Lam& lam, const Jac& jac) {
    double acc = sigma * grad_c;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
    for (int e = beg; e < end; ++e) acc = fm_fma(lam(e), jac(e), acc);
    return acc;
}

}  // namespace hipnlp
