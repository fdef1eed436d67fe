// knot_stage.h — what every kernel that runs a knot program does in front of the program, once (device code only; hipnlp.hip,
// hipnlp_pose.hip): the LDS-only barrier, the workgroup -> knot map, the staging of the knot records and tables, the dispatch of the
// per-wave program instances, and — for the two kernels that run the Hessian program — the scratch prefix and the multiplier gather.
// The kernels keep their own tables, hooks, programs and epilogues.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "layout.h"

namespace hipnlp {

// Workgroup barrier that orders LDS traffic only.  The phases of the knot program exchange data through LDS and through nothing
// else, so global loads may stay in flight across it: __syncthreads() carries a workgroup fence whose s_waitcnt vmcnt(0) makes every
// barrier wait for the copy-out tables prefetched at the top of the kernel.  (The "memory" clobber keeps the compiler from moving
// memory operations across it; the hardware wait covers the LDS operations of this wave.)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// workgroup -> knot, XCD-aware: workgroups are dealt round-robin over the 8 XCDs (observed, relied on for speed only), each with
// its own L2, so within one trajectory (one grid row) the workgroups x, x + 8, x + 16, ... share an XCD: they get CONSECUTIVE
// knots.  The neighbour record x_{k-1} every knot reads is then found in the L2 its owner just filled, and the short runs that
// neighbouring knots write into one 128-byte line of a constraint block of g meet in one L2 before they leave for HBM
// (measured, 100 knots x 64, HBM bytes per launch: 26.6 -> 16.5 MB read, 109.6 -> 96.1 MB written; algorithmic: 13.7 + 94.7 MB).
// A bijection for any row length: class j = x mod 8 owns q + (j < r) knots, q = nk / 8, r = nk mod 8.
__device__ __forceinline__ int xcd_knot(unsigned bx, unsigned nk) { return int((bx & 7u) * (nk >> 3) + min(bx & 7u, nk & 7u) + (bx >> 3)); }

// The knot program is instantiated ONCE PER WAVE (f: a generic lambda over the wave number as a compile-time constant: a task group is
// compiled into the one instance whose wave runs it) and dispatched by one switch, so that every wave executes a CONTIGUOUS
// instruction stream from the first phase to the last.  Written as `if (wave == w) { ... }` blocks phase after phase, every
// wave jumped over the other waves' code several times per phase, each jump a cold instruction-cache line.  The waves still meet
// at the same barriers: every instance contains all of them.
// (on the wave number as a SCALAR: dispatched on the per-lane value the switch is built out of execution masks — every instance skipped
//  by a branch on an empty mask — and the path that skips them all reaches the copy-out with a table fetch unconsumed: the wait that a
//  kernel's tables_are_here() moves in front of its early stores would be back in front of the final ones.  For the same reason the
//  last wave is the default: no path skips every instance.)
template <int WAVES, class F> __device__ __forceinline__ void dispatch_wave(int wave, F&& f) {
    static_assert(WAVES == 4 || WAVES == 8, "four or eight role-specialised waves");
    switch (__builtin_amdgcn_readfirstlane(wave)) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: if constexpr (WAVES == 8) { f(std::integral_constant<int, 3>{}); break; } [[fallthrough]];
        case 4: if constexpr (WAVES == 8) { f(std::integral_constant<int, 4>{}); break; } [[fallthrough]];
        case 5: if constexpr (WAVES == 8) { f(std::integral_constant<int, 5>{}); break; } [[fallthrough]];
        case 6: if constexpr (WAVES == 8) { f(std::integral_constant<int, 6>{}); break; } [[fallthrough]];
        default: f(std::integral_constant<int, WAVES - 1>{}); break;
    }
}

// ---- the knot records and the tables -> LDS ----------------------------------------------------------------------------------------
// Straight from global memory into LDS (global_load_lds_dwordx4: lane l of a wave delivers 16 bytes at LDS base + 16 l — no VGPR round
// trip, no ds_write; one instruction moves 1 KB), the 1 KB chunks of all blocks dealt round-robin over the waves.  (The previous
// version — every thread loads 8-byte words into registers and stores them to LDS — spent ~250 instructions per wave here, a tenth of
// the 100-knot launch.)
// Full layout: the whole HeadTables + GParams.  Compact layout: KSettings, the KinLite prefix of the kinematic tables and the
// GParamsLite prefix of the parameters.
//
// A kernel uses it in three steps, and keeps the wait between the last two in its own body:
//     KnotStage<WAVES> st(tid);
//     st.issue<COMPACT>(s, tabs, tb, x, pk, gp, b, k, N [, extra]);   // every staging load of the kernel is in flight
//     ... further loads of the kernel's own (copy-out tables, multipliers) ...
//     asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // the staging loads of THIS wave have landed in LDS
//     st.land(s);                                                     // what went through registers, the zero pads
//     lds_barrier();
// Scalars a kernel needs at its end are read BEFORE issue(): behind the direct loads the compiler no longer treats global memory as
// unwritten and would fetch them through vector registers.  What a kernel fetches into registers behind issue() is waited for with the
// staging loads (the compiler waits for EVERY outstanding load before an LDS access that follows a direct load) and may then stay in
// registers across the (LDS-only) barriers of the program.
struct KnotStageNoExtra { template <class St> __device__ __forceinline__ void operator()(St&) const {} };
template <int WAVES> struct KnotStage {
    static constexpr int WG = 64 * WAVES;
    // the record x_k is NXK = 189 doubles: 94 pieces + one double, which goes through a register like the periodicity variables below
    static constexpr int XB = NXK * 8 / 16 * 16, XREM = NXK - XB / 8;
    static_assert(XREM <= 1 && NXG * 8 % 16 == 0 && NXG <= 8, "record staging");
    static_assert(sizeof(KSettings) % 16 == 0 && sizeof(KinLite) % 16 == 0 && sizeof(GParamsLite) % 16 == 0 && sizeof(HeadTables) % 16 == 0 &&
                  sizeof(GParams) % 16 == 0 && (PK_STRIDE * 8) % 16 == 0, "staged in 16-byte pieces");
    const int tid, lane, wave_u;
    int rot = 0;
    int first = 0, ends = 0;        // this knot is the first one / the first or the last one of the horizon
    double xrem = 0.0, xov = 0.0;   // through registers: the odd last double of the two records; the periodicity variables of the other end
    __device__ __forceinline__ explicit KnotStage(int tid_) : tid(tid_), lane(tid_ & 63), wave_u(__builtin_amdgcn_readfirstlane(tid_ >> 6)) {}

    // a block of `bytes` (multiple of 16): wave (w + rot) mod WAVES moves the 1 KB chunk w of each round of WG x 16 bytes; `rot`
    // walks on by the chunks used, so that the small blocks land on different waves (everything here folds at compile time
    // except the wave number: no scalar branch, one predicated instruction per block and round)
    __device__ __forceinline__ void block(const void* src, void* dst, int bytes) {
        for (int r0 = 0; r0 < bytes; r0 += WG * 16) {
            const int wv = (wave_u + WAVES - rot % WAVES) & (WAVES - 1);
            const int off = r0 + wv * 1024 + lane * 16;
            if (off < bytes)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(static_cast<const char*>(src) + off),
                                                 (__attribute__((address_space(3))) void*)(static_cast<char*>(dst) + r0 + wv * 1024), 16, 0, 0);
            rot += ((bytes - r0 < WG * 16 ? bytes - r0 : WG * 16) + 1023) / 1024;
        }
    }

    // x: the trajectory's variables; pk, gp: the handle's parameter records ([batch][N][PK_STRIDE], [batch]); extra(*this): the blocks
    // only this kernel stages (block()), issued behind the tables and in front of the two register loads
    template <bool COMPACT, class Scratch, class Tabs, class Tables, class Extra = KnotStageNoExtra>
    __device__ __forceinline__ void issue(Scratch& s, Tabs& tabs, const Tables& tb, const double* x, const double* pk, const GParams* gp, int b, int k, int N,
                                          Extra extra = Extra()) {
        first = k == 0; ends = first || k == N - 1;
        block(x + size_t(NXK) * k, s.x, XB);
        if (!first) block(x + size_t(NXK) * (k - 1), s.xm, XB); else rot += (XB + 1023) / 1024;
        block(pk + (size_t(b) * N + k) * PK_STRIDE, s.pk, PK_STRIDE * 8);
        block(x + size_t(NXK) * N, s.xg, NXG * 8);
        if constexpr (COMPACT) {
            block(static_cast<const GParamsLite*>(gp + b), &tabs.gp, int(sizeof(GParamsLite)));
            block(&tb.head.ks, &tabs.ks, int(sizeof(KSettings)));
            block(static_cast<const KinLite*>(&tb.head.kt), &tabs.kt, int(sizeof(KinLite)));
        } else {
#ifdef HIPNLP_DIAG_LITE_STAGE
            // timing-only diagnostic build (wrong values): the full-layout kernels stage the lite tables only — 10.6 instead of 26.4 KB per
            // workgroup: what a shorter prologue could be worth on the 100-knot launch
            block(static_cast<const GParamsLite*>(gp + b), &tabs.gp, int(sizeof(GParamsLite)));
            block(static_cast<const KinLite*>(&tb.head.kt), &tabs.head.kt, int(sizeof(KinLite)));
            block(&tb.head.ks, &tabs.head.ks, int(sizeof(KSettings)));
#else
            block(gp + b, &tabs.gp, int(sizeof(GParams)));
            // (SPLIT: both halves stage every table.  The model-free half without the joint frames and link inertials it never reads — 5.2 of the
            //  8.4 KB — measured no different: 7.47 - 7.54 against 7.46 - 7.48 us per 100-knot launch)
            block(&tb.head, &tabs.head, int(sizeof(HeadTables)));
#endif
        }
        extra(*this);
        // through registers: the odd last double of the two records; horizon ends only: the periodicity variables of the other end (a
        // trimmed scratch has no room for them: its tasks read them from global memory, knot_body.h x_other)
        if (XREM && tid < 2 && !(first && tid == 1)) xrem = x[size_t(NXK) * (k - tid) + XB / 8];
        if constexpr (!Scratch::trimmed) { if (ends) { if (tid < NPER) xov = x[size_t(NXK) * (first ? N - 1 : 0) + periodicity_row_var(tid)]; } }
    }

    // behind the kernel's s_waitcnt vmcnt(0)
    template <class Scratch> __device__ __forceinline__ void land(Scratch& s) const {
        if constexpr (!Scratch::trimmed) { if (ends) { if (tid < NPER) s.xo[tid] = xov; } }
        if (XREM && tid < 2) (tid ? s.xm : s.x)[XB / 8] = xrem;
        if (first) { for (int i = tid; i < XB / 8; i += WG) s.xm[i] = 0.0; }
        // pads (no staging load touches them)
        if (tid >= 64 && tid < 64 + Scratch::xpad - NXK) { s.x[NXK + tid - 64] = 0.0; s.xm[NXK + tid - 64] = 0.0; }
        if (tid >= 128 && tid < 128 + 8 - NXG) s.xg[NXG + tid - 128] = 0.0;
    }
};

// ---- the kernels that run the Hessian program (hipnlp_knot_hess_kernel, hipnlp_knot_hvp_kernel) ----------------------------------------
// The Hessian program runs none of the tasks that emit Jacobian entries or the cost gradient: the last members of the knot scratch
// (grad, jac: 17.2 KB) are not allocated — a kernel declares BYTES of LDS and lays the scratch type over them.
template <class Scratch> struct HessScratchPrefix {
    static_assert(offsetof(Scratch, jac) + sizeof(Scratch::jac) + 16 > sizeof(Scratch) && offsetof(Scratch, grad) + sizeof(Scratch::grad) == offsetof(Scratch, jac),
                  "grad and jac are the last members of the scratch (up to tail padding)");
    static constexpr size_t BYTES = offsetof(Scratch, grad);
    static_assert(BYTES % 16 == 0, "scratch prefix");
    static_assert(!Scratch::trimmed && Scratch::xpad == XPAD, "the Hessian program runs on an untrimmed scratch: records of XPAD doubles");
};

// Multipliers of the rows this knot owns, by native slot (the same slot -> row map that scatters g), into the g staging area of
// the scratch (the Hessian program emits no g); of the next interval's angular momentum rows; the objective factor.  Two dependent global
// reads (row map, then multiplier): all row-map words first (the constructor, in front of the staging loads), all multipliers behind them
// (issue(), behind the staging loads) — two round trips, not two per iteration; store() behind the kernel's wait.
// G_USED: multipliers staged by native slot (compact scratch: gs::FIN, the horizon-end rows have no storage in g[]).
template <int G_USED, int WG = 256> struct MultiplierGather {
    static constexpr int LG_ITERS = (gs::COUNT + WG - 1) / WG;
    const int tid;
    int lga[LG_ITERS], lgb[LG_ITERS], nga = G_NONE, ngb = 0;
    double lv[LG_ITERS], lnext = 0.0, sig;
    template <class Tables> __device__ __forceinline__ MultiplierGather(const Tables& tb, const double* sigma, int b, int k, int N, int tid_) : tid(tid_) {
        const int v = k == 0 ? VAR_FIRST : (k == N - 1 ? VAR_LAST : VAR_INTERIOR);
#pragma unroll
        for (int it = 0; it < LG_ITERS; ++it) { lga[it] = tb.g_a[v][tid + it * WG]; lgb[it] = tb.g_b[tid + it * WG]; }   // (padded tables)
        if (tid < 3 && k + 1 < N) { const int slot = gs::HDYN + 3 + tid; nga = tb.g_a[k + 1 == N - 1 ? VAR_LAST : VAR_INTERIOR][slot]; ngb = tb.g_b[slot]; }
        sig = sigma[b];
    }
    __device__ __forceinline__ void issue(const double* lam /* of this trajectory */, int k) {
#pragma unroll
        for (int it = 0; it < LG_ITERS; ++it) lv[it] = lga[it] != G_NONE ? lam[lga[it] + lgb[it] * k] : 0.0;
        lnext = nga != G_NONE ? lam[nga + ngb * (k + 1)] : 0.0;
    }
    template <class Scratch, class Hx> __device__ __forceinline__ void store(Scratch& s, Hx& hx) const {
#pragma unroll
        for (int it = 0; it < LG_ITERS; ++it) { const int slot = tid + it * WG; if (slot < G_USED) s.g[slot] = lv[it]; }
        if (tid < 3) hx.lam_next[tid] = lnext;
        if (tid == 0) hx.sigma = sig;
    }
};

}  // namespace hipnlp
