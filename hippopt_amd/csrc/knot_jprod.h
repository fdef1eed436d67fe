// knot_jprod.h — the products with a STORED value run of jac g:  J v  (and grad f . v) and  sigma grad f + J^T lambda  (hipnlp.hip
// hipnlp_jac_times_kernel, hipnlp_jac_transpose_times_kernel; the test-only CPU emulation runs the same code).  No knot program: the
// values are whatever hipnlp_eval_device of the handle left in memory, the sums are table-driven.
//
// The columns of jac g are knot-local (knot_lgrad.h): the transpose product is the column sum of lgrad_column with the native slot of an
// entry replaced by its position in the knot's block of the value run.  The ROWS are not: a trapezoid-defect row of knot k has entries in
// the blocks of knot k - 1 and of knot k, a periodicity row in the blocks of both horizon ends, the x_0 momentum rows reach the
// horizon-global columns.  Layout::build gives every row ONE owner knot and lists, per variant of the pair (own block, predecessor's
// block), the entries of every owned row in ascending global column as (staged value, staged element of v).
#pragma once
#include <cstdint>

#include "knot_lgrad.h"

namespace hipnlp {

// pair variants: which tables a knot's workgroup reads.  The first block has another length and order than an interior one, so the knot
// behind the first one, a plain interior knot and the last knot all differ (the last knot's predecessor is whatever the layout says).
enum PairVariant : int { PV_FIRST = 0, PV_SECOND = 1, PV_INTERIOR = 2, PV_LAST = 3, PV_COUNT = 4 };

// What a workgroup of 256 threads stages, and Layout::build checks a handle's tables against:
//   values: the own block and the predecessor's block (JP_BLOCK_CAP each: seven per thread, the capacity of the Lagrangian-gradient
//           kernel), the entries of the other horizon end the last knot needs, the horizon-global run (knot 0);
//   v:      the records of the own knot, the predecessor and the other horizon end (JP_V_STRIDE apart), then the globals;
//   rows:   two per thread;   entry words: JP_WORDS_PER_THREAD per thread.
constexpr int JP_WG = 256;
constexpr int JP_BLOCK_CAP = LG_ENT_CAP;
constexpr int JP_OTHER_CAP = 128, JP_GLOB_CAP = 16;
constexpr int JP_POS_PRED = JP_BLOCK_CAP, JP_POS_OTHER = 2 * JP_BLOCK_CAP, JP_POS_GLOB = JP_POS_OTHER + JP_OTHER_CAP;
constexpr int JP_VALUES = JP_POS_GLOB + JP_GLOB_CAP;
constexpr int JP_V_STRIDE = 192, JP_V_PRED = JP_V_STRIDE, JP_V_OTHER = 2 * JP_V_STRIDE, JP_V_GLOB = 3 * JP_V_STRIDE;
constexpr int JP_V_WORDS = JP_V_GLOB + 8;
constexpr int JP_ROW_CAP = 2 * JP_WG;
constexpr int JP_WORDS_PER_THREAD = 8;
constexpr int JP_ENT_CAP = JP_WORDS_PER_THREAD * JP_WG;
// an entry word: staged value in bits 0..11, staged element of v in bits 12..; a row word: first entry in bits 0..11, entries in bits 12..
constexpr int JP_POS_BITS = 12, JP_CNT_MAX = 1023;
constexpr int32_t JP_POS_MASK = (1 << JP_POS_BITS) - 1;
static_assert(JP_VALUES <= (1 << JP_POS_BITS) && JP_ENT_CAP <= (1 << JP_POS_BITS) && JP_V_WORDS < (1 << (31 - JP_POS_BITS)), "jprod words");
static_assert(NXK <= JP_V_STRIDE && NXG <= 8 && NXG <= JP_GLOB_CAP, "staged records of v");

// One entry of an owned row: the staged value (JP_POS_*) and the staged element of v (JP_V_*).
struct JprodEntry { int32_t pos, var; };
HD constexpr int32_t jp_word(int pos, int var) { return int32_t(pos) | (int32_t(var) << JP_POS_BITS); }

struct alignas(16) JprodTables {
    int32_t word[PV_COUNT][JP_ENT_CAP];     // entry e: staged value | staged element of v << JP_POS_BITS   (0 behind the last entry)
    int32_t rdir[PV_COUNT][JP_ROW_CAP];     // owned row q: first entry | entries << JP_POS_BITS            (0 behind the last row)
    int32_t row_a[PV_COUNT][JP_ROW_CAP];    // owned row q of knot k is row row_a + row_b k of g             (G_NONE behind the last row)
    int32_t row_b[PV_COUNT][JP_ROW_CAP];
    int32_t other[JP_OTHER_CAP];            // the last knot: positions in knot 0's block of the entries it stages (-1 behind)
};

// (J v)_i: from +0.0, one fused multiply-add per entry [beg, end) in the order of the table (ascending global column).
// val(e) / vec(e): the value of entry e and its element of v, wherever the caller keeps them.
template <class Val, class Vec> HD double jprod_row(int beg, int end, const Val& val, const Vec& vec) {
    double acc = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
    for (int e = beg; e < end; ++e) acc = fm_fma(val(e), vec(e), acc);
    return acc;
}
// ... from staged words w, values jv and records vs
HD double jprod_row_staged(int32_t dir, const int32_t* w, const double* jv, const double* vs) {
    const int beg = dir & JP_POS_MASK, end = beg + (dir >> JP_POS_BITS);
    return jprod_row(beg, end, [&](int e) { return jv[w[e] & JP_POS_MASK]; }, [&](int e) { return vs[w[e] >> JP_POS_BITS]; });
}

// A column of  sigma grad f + J^T lambda:  sigma grad_c first (+0.0 without a gradient), then one fused multiply-add per entry in
// (column, row) order — lgrad_column over words whose low bits are positions in the knot's block of the value run.
HD double jprod_column_staged(bool with_grad, double sigma, double grad_c, int beg, int end, const int32_t* w, const double* lam, const double* jv) {
    return lgrad_column(with_grad ? sigma : 0.0, with_grad ? grad_c : 0.0, beg, end, [&](int e) { return lam[w[e] >> LG_SLOT_BITS]; },
                        [&](int e) { return jv[w[e] & ((1 << LG_SLOT_BITS) - 1)]; });
}

// grad f . v of one knot: the products of the knot's NXK variables (one per thread, +0.0 behind them) summed in the tree of a workgroup
// of four waves of 64 — a butterfly over the lanes (xor 1, 2, .. 32), then the waves in order.  prod: [JP_WG], overwritten.
HD double jprod_dot_product(double g, double v) { return fm_fma(g, v, 0.0); }
inline double jprod_dot_tree(double* prod) {
    double tmp[64];
    double waves[JP_WG / 64];
    for (int w = 0; w < JP_WG / 64; ++w) {
        double* a = prod + 64 * w;
        for (int s = 1; s < 64; s <<= 1) {
            for (int i = 0; i < 64; ++i) tmp[i] = a[i] + a[i ^ s];
            for (int i = 0; i < 64; ++i) a[i] = tmp[i];
        }
        waves[w] = a[0];
    }
    return ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

}  // namespace hipnlp
