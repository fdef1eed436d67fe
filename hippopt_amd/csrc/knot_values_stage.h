// knot_values_stage.h — what every kernel that works from STORED value runs of jac g and of the Hessian does in front of its sums, once
// (device code only; hipnlp.hip: hipnlp_hess_times_kernel, hipnlp_jac_times_kernel, hipnlp_jac_transpose_times_kernel, the KKT operator
// and its MINRES apply launch, hipnlp_saddle_diag_kernel): the dimensions of the runs, the table variant of a knot, the staging into LDS,
// the workgroup tree.  The sibling of knot_stage.h for the kernels that run no knot program; they keep their LDS arrays (and the overlays
// KK_* / SD_*), their tables, their sums and their stores.
// Every stage has the shape of KnotStage: issue(...) requests the loads into members that stay in registers (compile-time trip counts:
// nothing goes to scratch), land(...) writes them to the LDS bases the kernel passes.  A kernel calls every issue() before the first
// land(): all its staging loads are in one memory round trip; only loads addressed by table words (the multipliers, d_c) wait for those
// words.  No stage holds a barrier.  The test-only emulations state the same staging in their own words and do not include this header.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "knot_hess_layout.h"
#include "knot_kkt.h"
#include "layout.h"

namespace hipnlp {

// ---- the runs ------------------------------------------------------------------------------------------------------------------------
// A value run of jac g: the blocks of the knots (first, interior ..., last), then the horizon-global run.  Embedded in the kernels'
// argument structs behind the pointers (the first 64 bytes of an argument struct keep their offsets: the order here is theirs).
struct JacRunDims {
    int32_t N, n, m, nnz_first, nnz_interior, nnz_last, nnz_glob;
    int64_t nnz, glob_base;
    // (the three lengths are read first: from a choice between the MEMBERS the compiler makes a choice between their addresses, and a
    //  kernel then fetches every argument where a branch first needs it instead of all of them at entry)
    __host__ __device__ __forceinline__ int block_len(int k) const {
        const int first = nnz_first, interior = nnz_interior, last = nnz_last;
        return k == 0 ? first : (k == N - 1 ? last : interior);
    }
    __host__ __device__ __forceinline__ int64_t block_base(int k) const { return k == 0 ? int64_t(0) : int64_t(nnz_first) + int64_t(k - 1) * nnz_interior; }
};
// A value run of the Hessian: N blocks of nnz_knot entries, then the n_couple coupling values of the horizon ends.
struct HessRunDims { int32_t nnz_knot, n_couple; int64_t nnz_h; };
// which tables a knot reads: of the pair (own block, predecessor's block) — JprodTables — and of the own block — LgradTables
__host__ __device__ __forceinline__ constexpr int pair_variant(int k, int N) { return k == 0 ? PV_FIRST : (k == N - 1 ? PV_LAST : (k == 1 ? PV_SECOND : PV_INTERIOR)); }
__host__ __device__ __forceinline__ constexpr int block_variant(int k, int N) { return k == 0 ? VAR_FIRST : (k == N - 1 ? VAR_LAST : VAR_INTERIOR); }

// ---- the rows of jac g: own block, predecessor's block, the extras, the row entry words -> js [JP_VALUES], tw [JP_ENT_CAP] -----------
struct JacRowStage {
    static constexpr int WG = JP_WG, JB = JP_BLOCK_CAP / WG;
    static_assert(JP_BLOCK_CAP % WG == 0 && JP_OTHER_CAP <= WG && JP_GLOB_CAP <= WG && JP_ROW_CAP == 2 * WG, "jprod staging by 256 threads");
    static_assert(JP_POS_GLOB == JP_POS_OTHER + JP_OTHER_CAP, "the extra runs are staged side by side");
    const int tid;
    double o[JB], p[JB];
    double ex = 0.0;   // the entries of knot 0's block a last knot needs (threads 0 ..), the horizon-global run at knot 0 (threads 128 ..)
    int32_t wr[JP_WORDS_PER_THREAD];
    __device__ __forceinline__ explicit JacRowStage(int tid_) : tid(tid_) {}
    __device__ __forceinline__ void issue(const JprodTables& jt, const JacRunDims& d, const double* vals /* of this trajectory */, int k) {
        const int first = k == 0, last = k == d.N - 1;
        const int n_own = d.block_len(k), n_pred = first ? 0 : d.block_len(k - 1);
        const double* own = vals + d.block_base(k);
        const double* pred = vals + d.block_base(first ? 0 : k - 1);
#pragma unroll
        for (int it = 0; it < JB; ++it) { const int i = tid + it * WG; o[it] = i < n_own ? own[i] : 0.0; }
#pragma unroll
        for (int it = 0; it < JB; ++it) { const int i = tid + it * WG; p[it] = i < n_pred ? pred[i] : 0.0; }
        if (tid < JP_OTHER_CAP) {
            const int32_t q = jt.other[tid];
            if (last && q >= 0 && q < d.nnz_first) ex = vals[q];
        } else if (tid - JP_OTHER_CAP < JP_GLOB_CAP) {
            const int i = tid - JP_OTHER_CAP;
            if (first && i < d.nnz_glob) ex = vals[d.glob_base + i];
        }
        const int pv = pair_variant(k, d.N);
#pragma unroll
        for (int it = 0; it < JP_WORDS_PER_THREAD; ++it) wr[it] = jt.word[pv][tid + it * WG];
    }
    __device__ __forceinline__ void land(double* js, int32_t* tw) const {
#pragma unroll
        for (int it = 0; it < JB; ++it) { js[tid + it * WG] = o[it]; js[JP_POS_PRED + tid + it * WG] = p[it]; }
#pragma unroll
        for (int it = 0; it < JP_WORDS_PER_THREAD; ++it) tw[tid + it * WG] = wr[it];
        if (tid < JP_OTHER_CAP + JP_GLOB_CAP) js[JP_POS_OTHER + tid] = ex;
    }
};
// ---- four records in the JP_V_* arrangement: own knot, predecessor, other horizon end (last knot), the globals -> [JP_V_WORDS] --------
// Threads 0 .. JP_V_STRIDE - 1 carry one element of each knot record, the threads behind them one global element in r0; zeros where a
// record does not exist.  issue() loads a vector [n] of this trajectory; land() takes the thread's three values from wherever they come.
struct RecordStage {
    static_assert(JP_V_STRIDE + (JP_V_WORDS - JP_V_GLOB) <= JP_WG && JP_WG / 64 == 4, "records staged by 256 threads: four waves (workgroup_tree)");
    const int tid;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    __device__ __forceinline__ explicit RecordStage(int tid_) : tid(tid_) {}
    __device__ __forceinline__ void issue(const double* vb, int k, int N) {
        if (tid < NXK) {
            r0 = vb[int64_t(NXK) * k + tid];
            if (k != 0) r1 = vb[int64_t(NXK) * (k - 1) + tid];
            if (k == N - 1) r2 = vb[tid];
        } else if (tid >= JP_V_STRIDE && tid - JP_V_STRIDE < NXG) r0 = vb[int64_t(NXK) * N + (tid - JP_V_STRIDE)];
    }
    __device__ __forceinline__ void land(double* vs, double v0, double v1, double v2) const {
        if (tid < JP_V_STRIDE) { vs[tid] = v0; vs[JP_V_PRED + tid] = v1; vs[JP_V_OTHER + tid] = v2; }
        else if (tid - JP_V_STRIDE < JP_V_WORDS - JP_V_GLOB) vs[JP_V_GLOB + (tid - JP_V_STRIDE)] = v0;
    }
};
// ---- the columns of jac g: the own block's column words, the column of the thread, the multipliers, the last knot's global run -------
// -> lw [LG_ENT_CAP + 16], ls [LG_LAM_CAP], jg [16].  The own block's VALUES are not staged here: the operator has them from JacRowStage.
// Tables: LgradTables with block positions for native slots.  The multipliers are addressed by table words: issue_rows() first, issue()
// among the other staging loads, issue_multipliers() behind them.
template <class Tables> struct JacColumnStage {
    static constexpr int WG = 256, JB = LG_ENT_CAP / WG, LQ = LG_LAM_CAP / WG;
    static_assert(LG_ENT_CAP % WG == 0 && LG_LAM_CAP % WG == 0 && JP_GLOB_CAP <= 16, "column staging by 256 threads");
    const int tid;
    int32_t la[LQ], lb[LQ], cw[JB], cwg, e0, e1;   // e0, e1: entries [e0, e1) of the column this thread sums
    double lv[LQ], og;
    __device__ __forceinline__ explicit JacColumnStage(int tid_) : tid(tid_) {}
    __device__ __forceinline__ void issue_rows(const Tables& lt, int bv) {
#pragma unroll
        for (int it = 0; it < LQ; ++it) { la[it] = lt.row_a[bv][tid + it * WG]; lb[it] = lt.row_b[bv][tid + it * WG]; }
    }
    __device__ __forceinline__ void issue(const Tables& lt, int bv, const JacRunDims& d, const double* vals, int k) {
        og = (k == d.N - 1 && tid < 16 && tid < d.nnz_glob) ? vals[d.glob_base + tid] : 0.0;
#pragma unroll
        for (int it = 0; it < JB; ++it) cw[it] = lt.word[bv][tid + it * WG];
        cwg = lt.word[bv][LG_ENT_CAP + (tid & 15)];
        e0 = lt.beg[bv][tid]; e1 = lt.end[bv][tid];
    }
    __device__ __forceinline__ void issue_multipliers(const double* lam, int k) {
#pragma unroll
        for (int it = 0; it < LQ; ++it) lv[it] = la[it] != G_NONE ? lam[la[it] + lb[it] * k] : 0.0;
    }
    __device__ __forceinline__ void land(int32_t* lw, double* ls, double* jg) const {
#pragma unroll
        for (int it = 0; it < JB; ++it) lw[tid + it * WG] = cw[it];
#pragma unroll
        for (int it = 0; it < LQ; ++it) ls[tid + it * WG] = lv[it];
        if (tid < 16) { jg[tid] = og; lw[LG_ENT_CAP + tid] = cwg; }
    }
};
// ---- the knot's block of the Hessian run, its touch words, the row word of the thread's variable, the coupling term of the ends ------
// -> hv [HB * 256], hw [HVP_WORD_CAP].  Tables: HvpTables.  vb: v of this trajectory (the other end's element of a coupled variable).
template <class Tables> struct HessBlockStage {
    static constexpr int WG = 256, HB = (hk::COUNT + WG - 1) / WG, WORDS = HVP_WORD_CAP / WG;
    const int tid;
    double h[HB], vo = 0.0, cpl = 0.0;
    int32_t hwr[WORDS], row;
    bool ends_coupled;
    __device__ __forceinline__ explicit HessBlockStage(int tid_) : tid(tid_) {}
    __device__ __forceinline__ void issue(const Tables& vt, const HessRunDims& d, const double* hvals, const double* vb, int k, int N) {
        const int first = k == 0, last = k == N - 1;
        const double* blk = hvals + int64_t(d.nnz_knot) * k;
#pragma unroll
        for (int it = 0; it < HB; ++it) { const int i = tid + it * WG; h[it] = i < d.nnz_knot ? blk[i] : 0.0; }
#pragma unroll
        for (int it = 0; it < WORDS; ++it) hwr[it] = vt.word_pos[tid + it * WG];
        row = vt.row[tid];
        ends_coupled = d.n_couple > 0 && (first || last);
        if (tid < NXK && ends_coupled && ((row >> HVP_COUPLED_BIT) & 1)) {
            vo = vb[int64_t(NXK) * (first ? N - 1 : 0) + tid];
            cpl = hvals[int64_t(d.nnz_knot) * N + vt.couple[tid]];
        }
    }
    __device__ __forceinline__ void land(double* hv, int32_t* hw) const {
#pragma unroll
        for (int it = 0; it < HB; ++it) hv[tid + it * WG] = h[it];
#pragma unroll
        for (int it = 0; it < WORDS; ++it) hw[tid + it * WG] = hwr[it];
    }
    // the row word hvp_thread_row takes: without the coupling bit away from the horizon ends
    __device__ __forceinline__ int32_t row_word() const { return ends_coupled ? row : row & ~(1 << HVP_COUPLED_BIT); }
};
// ---- the tree of jprod_dot_tree over a workgroup's 256 per-thread values: a butterfly over the lanes, then the four waves in order ----
// (every thread returns the sum; part: four doubles of LDS, one call per launch)
__device__ __forceinline__ double workgroup_tree(double acc, double* part) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, s, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

}  // namespace hipnlp
