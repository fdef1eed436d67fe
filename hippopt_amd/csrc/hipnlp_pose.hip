// hipnlp_pose.hip — gfx950 kernel and the C-ABI (include/hipnlp.h, hipnlp_pose_*) of the static pose finder NLP
// (BASELINE config 2; turnkey_planners/humanoid_pose_finder/planner.py:323-788).
//
// One 256-thread workgroup (four role-specialised wavefronts, pose_body.h HIPNLP_POSE_PROGRAM) per pose: the 81 variables are
// gathered into a knot record in LDS (velocities zero), the kinematic tasks of knot_body.h and the pose tasks fill the native
// g / jac / grad slots in LDS, and the workgroup streams out the pose's CCS value run, its rows of g, grad f and the cost terms.
// The total cost of a pose is summed inside the same workgroup in a fixed order (bitwise reproducible); no second kernel.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "knot_stage.h"
#include "pose_layout.h"
#include "pose_products.h"

// (hipnlp.hip: hipMemcpy that survives a host buffer inside a stale self-registered range)
extern "C" hipError_t hipnlp_internal_memcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind);

using namespace hipnlp;

namespace {

constexpr int WG = 256;
constexpr int XR_STRIDE = 64;
constexpr int POSE_MAX_NNZ = 1024;
constexpr int POSE_MAX_HNNZ = hs::COUNT;
constexpr int POSE_MAX_M = 256;   // one thread per row stages the multipliers (m = 89 .. 104 by mode)
static_assert(XR_COUNT <= XR_STRIDE, "pose reference record");

struct PoseTables {
    HeadTables head;
    int32_t g_row[gs::COUNT];
    int32_t jperm[POSE_MAX_NNZ];
    int32_t nnz, m;
    int32_t hperm[POSE_MAX_HNNZ];
    int32_t hnnz, pad_;
    PoseHands hands;
    int32_t row_slot[POSE_MAX_M];   // native g slot of row i (the inverse of g_row; -1 behind m): the Hessian kernel scatters the multipliers with it
};

struct PArgs {
    const PoseTables* tb;
    const double* x;    // [batch][81]
    const double* pk;   // [batch][PK_STRIDE]
    const double* xr;   // [batch][XR_STRIDE]
    const GParams* gp;  // [batch]
    double* f;          // [batch]           or null
    double* grad;       // [batch][81]       or null
    double* g;          // [batch][m]        or null
    double* jac;        // [batch][nnz]      or null
    double* cost_terms; // [batch][POSE_NCT]
    int32_t* flags;     // [batch]
    // Hessian kernel only
    const double* sigma;   // [batch]   objective factor
    const double* lambda;  // [batch][m]
    double* hess;          // [batch][hnnz]
    int32_t m;             // rows of one pose (a kernel argument: the address of a pose's multipliers does not wait for a table)
#ifdef HIPNLP_STAMPS
    unsigned long long* stamps;   // diagnostic build only (tools/diag/pose_stamps.py): [batch][4 waves][64] s_memtime words
#endif
};

constexpr int pose_jslots(int terrain) { return pjs::slots(terrain == HIPNLP_TERRAIN_PLANAR); }
template <int TERRAIN> struct PoseEm {
    static constexpr int kTerrain = TERRAIN;
    static constexpr bool kStatic = true;   // (knot_body.h em_static: the velocities of a pose are zero)
    using Scratch = KnotScratchT<LAYOUT_COMPACT, pose_jslots(TERRAIN), true>;   // (PoseScratchT below)
    double* g;
    double* jac;    // the staging (pose_body.h pjs): [per-point constants | kept global constants | varying regions]
    double* jacv;   // the same, moved back so that a native slot of the varying regions indexes it directly
    __device__ __forceinline__ void G(int slot, int, double v) { g[slot] = v; }
    __device__ __forceinline__ void J(int slot, int, int, double v) { jacv[slot] = v; }                 // (entries that depend on x: slots >= js::V0)
    __device__ __forceinline__ void JC(int slot, int, int, double v) { jac[pjs::index(slot)] = v; }     // (constants: any region)
    __device__ __forceinline__ void JD(int slot, int, int, double v) { jac[pjs::index(slot)] = v; }     // (the pose finder's own entries in slots of region D)
};

template <int TERRAIN> struct PoseHessEm {
    static constexpr int kTerrain = TERRAIN;
    static constexpr bool kStatic = true;
    using Scratch = KnotScratchT<LAYOUT_COMPACT_NOG, pose_jslots(TERRAIN), true>;   // (no row, no gradient entry is emitted: neither staging exists)
    double* g;
    double* jac;
    double* h;
    __device__ __forceinline__ void G(int slot, int, double v) { g[slot] = v; }
    __device__ __forceinline__ void J(int slot, int, int, double v) { jac[slot] = v; }
    __device__ __forceinline__ void H(int slot, int, int, double v) { h[slot] = v; }
};

// LDS of a pose workgroup: the COMPACT knot scratch (knot_body.h: own[] on the joint records, which are dead once the forward kinematics
// has read them) in its STATIC form (no velocity arrays, a 64-word reference record in place of the previous knot's), a Jacobian staging
// cut to the pieces the pose program touches (pose_body.h pjs), and the LITE tables of the four-wave callback kernels (the joint frames
// and link inertials, read once per pose, come from global memory) instead of the whole HeadTables: 31.8 KB on the planar terrain ->
// FIVE workgroups per CU (LDS is handed out in granules of 1 280 B: 25 granules each; 38.5 KB and four per CU until round 6).
template <int TERRAIN> using PoseScratchT = KnotScratchT<LAYOUT_COMPACT, pose_jslots(TERRAIN), true>;
static_assert(pose_jslots(HIPNLP_TERRAIN_SMOOTH_STEPS) != js::COUNT && pose_jslots(HIPNLP_TERRAIN_PLANAR) != js::vary_slots(false) && pose_jslots(HIPNLP_TERRAIN_SMOOTH_STEPS) != js::vary_slots(false),
              "pose scratch: trimmed (the hand tables live in the tables block), and hd[] (the hand buffer) must exist");

// the hand tables (224 B; read by several task groups of both kernels: an LDS copy, not a global load per use) live in the tables block (every
// pose scratch is a trimmed one since round 6; an untrimmed scratch would park them on the periodicity variables xo[] no pose task reads)
template <bool OWN_HANDS> struct PoseSharedT;
// (bad: the workgroup's non-finite vote — a word here instead of __syncthreads_or, whose reduction brings 256 B of LDS of its own)
template <> struct alignas(16) PoseSharedT<true> { KSettings ks; KinLite kt; GParamsLite gp; PoseHands hands; int32_t bad, pad_[3]; };
template <> struct alignas(16) PoseSharedT<false> { KSettings ks; KinLite kt; GParamsLite gp; int32_t bad, pad_[3]; };
// every wave ORs its vote into tabs.bad (cleared by pose_stage); returns the workgroup's vote in every thread
template <class T> __device__ __forceinline__ int pose_vote(T& tabs, int bad, int lane) {
    if (__any(bad) && lane == 0) tabs.bad = 1;   // (all writers store the same value)
    __syncthreads();
    return tabs.bad;
}
static_assert(sizeof(PoseHands) % 8 == 0 && sizeof(PoseHands) <= sizeof(double) * NPER, "staged as 8-byte words; fits on xo[]");
template <class S, class T> __device__ __forceinline__ PoseHands* pose_hands(S& s, T& tabs) {
    if constexpr (S::trimmed) return &tabs.hands;
    else return reinterpret_cast<PoseHands*>(s.xo);
}

// tables, parameters and the pose's variables -> LDS (ends with a workgroup barrier)
struct PoseStageNoMid { __device__ __forceinline__ void operator()() const {} };
template <class S, class T, class Mid = PoseStageNoMid> __device__ __forceinline__ void pose_stage(const PArgs& a, S& s, T& tabs, int b, int tid, Mid mid = Mid()) {
    const PoseTables& tb = *a.tb;
    // every global load in flight before the first LDS store waits for one (see hipnlp_knot_kernel).  Four pieces, as 8-byte words:
    // settings | lite kinematic tables (the KinLite prefix of the full ones) | lite parameters of this pose | hand tables
    constexpr int W0 = int(sizeof(KSettings) / 8), W1 = W0 + int(sizeof(KinLite) / 8), W2 = W1 + int(sizeof(GParamsLite) / 8), W3 = W2 + int(sizeof(PoseHands) / 8);
    constexpr int T_ITERS = (W3 + WG - 1) / WG;
    static_assert(sizeof(KSettings) % 8 == 0 && sizeof(KinLite) % 8 == 0 && sizeof(GParamsLite) % 8 == 0, "copied in 8-byte words");
    static_assert(S::xpad <= WG && PK_STRIDE <= WG && POSE_NX <= WG && POSE_MAX_NNZ % WG == 0 && XR_STRIDE <= S::xm_len, "one record word per thread");
    const double* src0 = reinterpret_cast<const double*>(&tb.head.ks);
    const double* src1 = reinterpret_cast<const double*>(static_cast<const KinLite*>(&tb.head.kt));
    const double* src2 = reinterpret_cast<const double*>(static_cast<const GParamsLite*>(a.gp + b));
    const double* src3 = reinterpret_cast<const double*>(&tb.hands);
    double* dst0 = reinterpret_cast<double*>(&tabs.ks);
    double* dst1 = reinterpret_cast<double*>(&tabs.kt);
    double* dst2 = reinterpret_cast<double*>(&tabs.gp);
    double* dst3 = reinterpret_cast<double*>(pose_hands(s, tabs));
    double tv[T_ITERS];
#pragma unroll
    for (int it = 0; it < T_ITERS; ++it) {
        const int i = tid + it * WG;
        tv[it] = i < W0 ? src0[i] : (i < W1 ? src1[i - W0] : (i < W2 ? src2[i - W1] : (i < W3 ? src3[i - W2] : 0.0)));
    }
    const double xrv = tid < XR_STRIDE ? a.xr[size_t(b) * XR_STRIDE + tid] : 0.0;
    const double pkv = tid < PK_STRIDE ? a.pk[size_t(b) * PK_STRIDE + tid] : 0.0;
    const double xval = tid < POSE_NX ? a.x[size_t(b) * POSE_NX + tid] : 0.0;
#pragma unroll
    for (int it = 0; it < T_ITERS; ++it) {
        const int i = tid + it * WG;
        if (i < W0) dst0[i] = tv[it]; else if (i < W1) dst1[i - W0] = tv[it]; else if (i < W2) dst2[i - W1] = tv[it]; else if (i < W3) dst3[i - W2] = tv[it];
    }
    if (tid < S::xpad) s.x[tid] = 0.0;
    if (tid < XR_STRIDE) s.xm[tid] = xrv;
    if (tid < PK_STRIDE) s.pk[tid] = pkv;
    if (tid == 0) tabs.bad = 0;
    __syncthreads();
    if (tid < POSE_NX) s.x[pose_to_knot_col(tid)] = xval;
    mid();   // (LDS stores of the caller that must follow stores it made before the call)
    __syncthreads();
}

// Planar terrain: FIVE workgroups per CU (<= 96 VGPRs: 90 used since the static kinematics; <= 32 000 B of LDS); smooth steps: four (123 VGPRs).
template <int TERRAIN> __global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 4, TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 4)))
void hipnlp_pose_kernel(PArgs a) {
    using Scratch = PoseScratchT<TERRAIN>;
    static_assert(std::is_same_v<Scratch, typename PoseEm<TERRAIN>::Scratch>, "the emitter names the scratch the tasks run on");
    __shared__ Scratch s;
    __shared__ PoseSharedT<Scratch::trimmed> tabs;
    static_assert(sizeof(Scratch) + sizeof(PoseSharedT<Scratch::trimmed>) <= (TERRAIN == HIPNLP_TERRAIN_PLANAR ? 32000 : 40960), "five / four workgroups per CU");
#ifdef HIPNLP_STAMPS
    const unsigned long long st_entry = __builtin_amdgcn_s_memtime();
#endif
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x;
    const PoseTables& tb = *a.tb;
    pose_stage(a, s, tabs, b, tid);
#ifdef HIPNLP_STAMPS
    const unsigned long long st_staged = __builtin_amdgcn_s_memtime();
    unsigned long long st_arr[8], st_dep[8], st_task[24];
    int st_nb = 0, st_nt = 0;
#endif
    // copy-out tables (CCS permutation, g row map): fetched now, consumed at the very end
    constexpr int JP_ITERS = (POSE_MAX_NNZ + WG - 1) / WG, GR_ITERS = (gs::COUNT + WG - 1) / WG;
    int32_t jp[JP_ITERS], gr[GR_ITERS];
#pragma unroll
    for (int it = 0; it < JP_ITERS; ++it) jp[it] = tb.jperm[tid + it * WG];          // (POSE_MAX_NNZ is a multiple of the workgroup)
#pragma unroll
    for (int it = 0; it < GR_ITERS; ++it) { const int slot = tid + it * WG; gr[it] = slot < gs::COUNT ? tb.g_row[slot] : -1; }
    const int nnz = tb.nnz, m = tb.m;

    KnotInfo ki{1, 3, 0, 0};   // "interior knot": the k >= 1 rows / costs of the shared tasks are active
    PoseEm<TERRAIN> em{s.g, s.jac, s.jac - (js::V0 - pjs::DSLOTS)};
    Ctx<PoseEm<TERRAIN>> cx(s, tabs.kt, tabs.ks, tabs.gp, ki, em, &tb.head.kt, a.gp + b);   // (full tables: global memory)
    cx.hands = pose_hands(s, tabs);
    // (one contiguous program instance per wave, see knot_stage.h dispatch_wave: no wave jumps over the other waves' code)
#ifdef HIPNLP_STAMPS
#define DEV_R(w, w8, fn, nt) if constexpr ((w) == W) { for (int t_ = lane; t_ < (nt); t_ += 64) fn(cx, t_); if (st_nt < 24) st_task[st_nt++] = __builtin_amdgcn_s_memtime(); }
#define DEV_BARRIER st_arr[st_nb] = __builtin_amdgcn_s_memtime(); lds_barrier(); st_dep[st_nb] = __builtin_amdgcn_s_memtime(); st_nb++;
#elif defined(HIPNLP_TASK_MARKS)
    // diagnostic compile (assembly only, never a library): comment markers around every task group for tools/diag/isa_mix.py / reading the ISA
#define DEV_R(w, w8, fn, nt) if constexpr ((w) == W) { asm volatile("; TASK_BEGIN " #fn); for (int t_ = lane; t_ < (nt); t_ += 64) fn(cx, t_); asm volatile("; TASK_END " #fn); }
#define DEV_BARRIER lds_barrier();
#else
#define DEV_R(w, w8, fn, nt) if constexpr ((w) == W) { for (int t_ = lane; t_ < (nt); t_ += 64) fn(cx, t_); }
#define DEV_BARRIER lds_barrier();
#endif
    auto run_wave = [&](auto wc) __attribute__((always_inline)) {
        constexpr int W = decltype(wc)::value;
        HIPNLP_POSE_PROGRAM(DEV_R, DEV_BARRIER)
    };
    switch (wave) {   // (on the per-lane value, as these kernels always have: the scalar switch of dispatch_wave lays their instances out anew)
        case 0: run_wave(std::integral_constant<int, 0>{}); break;
        case 1: run_wave(std::integral_constant<int, 1>{}); break;
        case 2: run_wave(std::integral_constant<int, 2>{}); break;
        default: run_wave(std::integral_constant<int, 3>{}); break;
    }
#undef DEV_R
#undef DEV_BARRIER

    // copy-out: every LDS read in flight before the first store (as read -> wait -> store per piece, behind a branch each, the eight
    // pieces went one after the other: 2.3 k cycles at batch against 0.9 k in the Hessian kernel, which has two)
    int bad = 0;
    double jv[JP_ITERS], gv[GR_ITERS];
#pragma unroll
    for (int it = 0; it < JP_ITERS; ++it) jv[it] = s.jac[jp[it]];                    // (the table holds STAGING indices, pjs::index; behind nnz: 0)
#pragma unroll
    for (int it = 0; it < GR_ITERS; ++it) gv[it] = s.g[gr[it] >= 0 ? tid + it * WG : 0];
    const double gradv = s.grad[pose_to_knot_col(tid < POSE_NX ? tid : 0)];
    const double costv = pose_cost_terms_out(s)[tid < POSE_NCT ? tid : 0];           // (t_pose_cost_total: the nine terms side by side)
    const double tot = s.cost[CT_POSE_TOTAL];                                         // (and their sum, in their order)
    if (a.jac) {
        double* out = a.jac + size_t(b) * nnz;
#pragma unroll
        for (int it = 0; it < JP_ITERS; ++it) { const int e = tid + it * WG; if (e < nnz) { bad |= !isfinite(jv[it]); out[e] = jv[it]; } }
    }
    if (a.g) {
        double* out = a.g + size_t(b) * m;
#pragma unroll
        for (int it = 0; it < GR_ITERS; ++it) if (gr[it] >= 0) { bad |= !isfinite(gv[it]); out[gr[it]] = gv[it]; }
    }
    if (a.grad && tid < POSE_NX) { bad |= !isfinite(gradv); a.grad[size_t(b) * POSE_NX + tid] = gradv; }
    if (tid < POSE_NCT) a.cost_terms[size_t(b) * POSE_NCT + tid] = costv;
    if (tid == 0) {
        bad |= !isfinite(tot);
        if (a.f) a.f[b] = tot;
    }
    const int anybad = pose_vote(tabs, bad, lane);
    if (tid == 0) a.flags[b] = anybad;
#ifdef HIPNLP_STAMPS
    if (a.stamps && lane == 0) {   // [0] entry [1] staged [2] barriers [3] task groups [4] end | [8 + 2 i] arrival at / [9 + 2 i] departure from barrier i | [32 + t] end of task group t
        unsigned long long* o = a.stamps + (size_t(b) * 4 + wave) * 64;
        o[0] = st_entry; o[1] = st_staged; o[2] = st_nb; o[3] = st_nt; o[4] = __builtin_amdgcn_s_memtime();
        for (int i = 0; i < st_nb; ++i) { o[8 + 2 * i] = st_arr[i]; o[9 + 2 * i] = st_dep[i]; }
        for (int i = 0; i < st_nt; ++i) o[32 + i] = st_task[i];
    }
#endif
}

// Exact Hessian of the Lagrangian (IPOPT eval_h, pose_hess_body.h): the pose program runs as in hipnlp_pose_kernel (its g / jac
// values stay in LDS, unused), the Hessian tasks run behind it and the workgroup streams out the lower-triangle CCS value run.
// The Hessian program runs none of the tasks that emit Jacobian entries: the jac staging area (the last 13.8 / 15.7 KB of the scratch) is
// not allocated.
// Workgroups per CU (round 6): the scratch ends in front of the gradient and carries no staging of g (the Hessian program emits neither), the
// (q_b, q_b) block is formed by three small task groups instead of one that held 124 registers: 31.0 KB and 92 VGPRs on the planar terrain ->
// FIVE workgroups per CU (25 granules of 1 280 B, 96 registers); the smooth terrain's kernel (158 VGPRs for the second-order jets) stays at three.
template <int TERRAIN> __global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 3, TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 3)))
void hipnlp_pose_hess_kernel(PArgs a) {
    using Scratch = typename PoseHessEm<TERRAIN>::Scratch;
    static_assert(offsetof(Scratch, jac) + sizeof(Scratch::jac) + 16 > sizeof(Scratch) && offsetof(Scratch, grad) + sizeof(Scratch::grad) == offsetof(Scratch, jac),
                  "grad and jac are the last two members of the scratch (up to tail padding)");
    __shared__ alignas(16) double s_raw[offsetof(Scratch, grad) / sizeof(double)];
    Scratch& s = *reinterpret_cast<Scratch*>(s_raw);
    __shared__ PoseSharedT<Scratch::trimmed> tabs;
    __shared__ HessScratch hx;
#ifdef HIPNLP_STAMPS
    const unsigned long long st_entry = __builtin_amdgcn_s_memtime();
#endif
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x;
    const PoseTables& tb = *a.tb;
    // the multiplier of every native g slot: thread i fetches the multiplier of ROW i and the slot that row lives in — two independent
    // loads, in flight together with the staging loads below — and scatters it between the two barriers of the staging, over zeros.
    // (Until round 6: slot -> row -> multiplier, two dependent round trips in front of the staging: 6.1 k cycles of a 21.8 k cycle pose.)
    const int m = a.m;
    double lam_i = 0.0, sig = 0.0;
    int slot_i = -1;
    if (tid < m) { lam_i = a.lambda[size_t(b) * m + tid]; slot_i = tb.row_slot[tid]; }
    if (tid == 0) sig = a.sigma[b];
    for (int slot = tid; slot < gs::COUNT; slot += WG) hx.lam[slot] = 0.0;
    pose_stage(a, s, tabs, b, tid, [&]() { if (slot_i >= 0) hx.lam[slot_i] = lam_i; if (tid == 0) hx.sigma = sig; });
#ifdef HIPNLP_STAMPS
    const unsigned long long st_staged = __builtin_amdgcn_s_memtime();
    unsigned long long st_arr[10], st_dep[10], st_task[24];
    int st_nb = 0, st_nt = 0;
#endif

    constexpr int HP_ITERS = (POSE_MAX_HNNZ + WG - 1) / WG;
    int32_t hp[HP_ITERS];
#pragma unroll
    for (int it = 0; it < HP_ITERS; ++it) { const int e = tid + it * WG; hp[it] = e < POSE_MAX_HNNZ ? tb.hperm[e] : 0; }   // (copy-out permutation, consumed at the end)
    const int hnnz = tb.hnnz;
    KnotInfo ki{1, 3, 0, 0};
    PoseHessEm<TERRAIN> em{nullptr, nullptr, hx.H};   // (no task of the Hessian program emits a row or a Jacobian entry)
    Ctx<PoseHessEm<TERRAIN>> cx(s, tabs.kt, tabs.ks, tabs.gp, ki, em, &tb.head.kt, a.gp + b);
    cx.hands = pose_hands(s, tabs);
    HCtx<PoseHessEm<TERRAIN>> hcx{cx, hx};
    // (one contiguous program instance per wave, see knot_stage.h dispatch_wave: no wave jumps over the other waves' code)
#ifdef HIPNLP_STAMPS
#define DEV_KIN(w, fn, nt) if constexpr ((w) == W) { for (int t_ = lane; t_ < (nt); t_ += 64) fn(cx, t_); if (st_nt < 24) st_task[st_nt++] = __builtin_amdgcn_s_memtime(); }
#define DEV_RH(w, fn, nt) if constexpr ((w) == W) { for (int t_ = lane; t_ < (nt); t_ += 64) fn(hcx, t_); if (st_nt < 24) st_task[st_nt++] = __builtin_amdgcn_s_memtime(); }
#define DEV_BARRIER st_arr[st_nb] = __builtin_amdgcn_s_memtime(); lds_barrier(); st_dep[st_nb] = __builtin_amdgcn_s_memtime(); st_nb++;
#else
#define DEV_KIN(w, fn, nt) if constexpr ((w) == W) { for (int t_ = lane; t_ < (nt); t_ += 64) fn(cx, t_); }
#define DEV_RH(w, fn, nt) if constexpr ((w) == W) { for (int t_ = lane; t_ < (nt); t_ += 64) fn(hcx, t_); }
#define DEV_BARRIER lds_barrier();
#endif
    auto run_wave = [&](auto wc) __attribute__((always_inline)) {
        constexpr int W = decltype(wc)::value;
        HIPNLP_POSE_HESS_PROGRAM(DEV_KIN, DEV_RH, DEV_BARRIER)
    };
    switch (wave) {   // (on the per-lane value, as these kernels always have: the scalar switch of dispatch_wave lays their instances out anew)
        case 0: run_wave(std::integral_constant<int, 0>{}); break;
        case 1: run_wave(std::integral_constant<int, 1>{}); break;
        case 2: run_wave(std::integral_constant<int, 2>{}); break;
        default: run_wave(std::integral_constant<int, 3>{}); break;
    }
#undef DEV_KIN
#undef DEV_RH
#undef DEV_BARRIER
    int bad = 0;
    double* out = a.hess + size_t(b) * hnnz;
#pragma unroll
    for (int it = 0; it < HP_ITERS; ++it) { const int e = tid + it * WG; if (e < hnnz) { const double v = hx.H[hp[it]]; bad |= !isfinite(v); out[e] = v; } }
    const int anybad = pose_vote(tabs, bad, lane);
    if (tid == 0) a.flags[b] = anybad;
#ifdef HIPNLP_STAMPS
    if (a.stamps && lane == 0) {
        unsigned long long* o = a.stamps + (size_t(b) * 4 + wave) * 64;
        o[0] = st_entry; o[1] = st_staged; o[2] = st_nb; o[3] = st_nt; o[4] = __builtin_amdgcn_s_memtime();
        for (int i = 0; i < st_nb; ++i) { o[8 + 2 * i] = st_arr[i]; o[9 + 2 * i] = st_dep[i]; }
        for (int i = 0; i < st_nt; ++i) o[32 + i] = st_task[i];
    }
#endif
}

// =====================================================================================================================
// The pose finder's products are workgroup-local (pose_products.h): a pose is ONE workgroup, which holds every entry of jac g in the cut
// staging when the pose program ends and every entry of the Hessian of the Lagrangian in hx.H when the Hessian program ends.  The three
// kernels below run those two programs unchanged — the same scratch, the same emitters, the same bits — and replace the copy-out by sums
// over the directories of PoseLayout::build_product_tables, one column / row / variable per thread: no atomics, no second pass, a fixed
// order.  81 (or m + 1) doubles leave per pose instead of up to 1 024 + m + 81 (or hnnz); neither jac g nor H is ever written.
// =====================================================================================================================
struct PPArgs {
    PArgs p;                    // what the pose kernels take: tables, x, parameters, flags; sigma, lambda and m as the Hessian kernel
    const PoseProdTables* pt;
    const double* v;            // [batch][81]       direction (jvp, hvp)
    double* out;                // [batch][81]       xbar (lgrad), H v (hvp);  [batch][m] J v (jvp) or null
    double* dot;                // [batch]           grad f . v (jvp) or null
};
constexpr int PP_LGRAD = 0, PP_JVP = 1;
// (a staging functor of their own, nothing to do in it: with PoseStageNoMid the first-order kernels would share hipnlp_pose_kernel's
//  instantiation of pose_stage, and the compiler then lays that kernel's staging out differently — same registers, other instructions)
struct PoseStageProducts { __device__ __forceinline__ void operator()() const {} };
constexpr int PP_EW = PP_ENT_CAP / WG, PP_TW = PP_TOUCH_CAP / WG;
constexpr int PP_DOT_THREAD = WG - 1;   // the lane that sums grad f . v (m = 89 .. 104 rows: a thread of the fourth wave, which sums no row)
static_assert(PP_WG == WG && PP_ENT_CAP == POSE_MAX_NNZ && PP_ROW_CAP == POSE_MAX_M, "pose_products.h counts in workgroups of this file");

// Where the first-order kernels stage once the pose program has ended.  Nothing reads the scratch then but the sums, which need grad and
// jac (these kernels store no g and no cost term): the multipliers / the direction go on the joint records and own[] (one union: read by
// the forward kinematics and the composites, phases two to four), the entry words on Rw, ow, aw and comp (contiguous doubles: the last
// reader of the kinematic arrays is the consistency-row phase, whose barrier is the program's last).
template <class S> __device__ __forceinline__ double* pose_factor_stage(S& s) { return lgrad_lam_stage(s); }
template <class S> __device__ __forceinline__ int32_t* pose_word_stage(S& s) { return reinterpret_cast<int32_t*>(&s.Rw[0][0]); }

// MODE PP_LGRAD: xbar = sigma grad f + J^T lambda, one thread per column.  MODE PP_JVP: J v, one thread per row, and grad f . v on one lane.
template <int TERRAIN, int MODE, class Scratch, class Tabs> __device__ __forceinline__ void pose_first_order(const PPArgs& pa, Scratch& s, Tabs& tabs) {
    static_assert(std::is_same_v<Scratch, typename PoseEm<TERRAIN>::Scratch>, "the emitter names the scratch the tasks run on");
    static_assert(PP_ROW_CAP * sizeof(double) <= sizeof(ScratchJrOwn<LAYOUT_COMPACT_NOG>), "multipliers / direction on the joint records");
    static_assert(offsetof(Scratch, comp) + sizeof(Scratch::comp) - offsetof(Scratch, Rw) >= PP_ENT_CAP * sizeof(int32_t) && offsetof(Scratch, comp) < offsetof(Scratch, grad), "entry words on Rw .. comp");
    const PArgs& a = pa.p;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x;
    const PoseTables& tb = *a.tb;
    const PoseProdTables& pt = *pa.pt;
    // the factor of this thread (the multiplier of ROW tid / element tid of v), sigma, the entry words and this thread's directory word:
    // independent loads, in flight together with the staging loads (as hipnlp_pose_hess_kernel loads its multipliers)
    const int m = a.m;
    double fac = 0.0, sig = 0.0;
    if constexpr (MODE == PP_LGRAD) { if (tid < m) fac = a.lambda[size_t(b) * m + tid]; sig = a.sigma[b]; }
    else { if (tid < POSE_NX) fac = pa.v[size_t(b) * POSE_NX + tid]; }
    int32_t w[PP_EW];
#pragma unroll
    for (int it = 0; it < PP_EW; ++it) w[it] = (MODE == PP_LGRAD ? pt.col_word : pt.row_word)[tid + it * WG];
    const int32_t dir = (MODE == PP_LGRAD ? pt.col_dir : pt.row_dir)[tid];
    pose_stage(a, s, tabs, b, tid, PoseStageProducts());

    KnotInfo ki{1, 3, 0, 0};
    PoseEm<TERRAIN> em{s.g, s.jac, s.jac - (js::V0 - pjs::DSLOTS)};
    Ctx<PoseEm<TERRAIN>> cx(s, tabs.kt, tabs.ks, tabs.gp, ki, em, &tb.head.kt, a.gp + b);
    cx.hands = pose_hands(s, tabs);
#define DEV_R(w, w8, fn, nt) if constexpr ((w) == W) { for (int t_ = lane; t_ < (nt); t_ += 64) fn(cx, t_); }
#define DEV_BARRIER lds_barrier();
    auto run_wave = [&](auto wc) __attribute__((always_inline)) {
        constexpr int W = decltype(wc)::value;
        HIPNLP_POSE_PROGRAM(DEV_R, DEV_BARRIER)
    };
    switch (wave) {   // (as hipnlp_pose_kernel: the same program instances)
        case 0: run_wave(std::integral_constant<int, 0>{}); break;
        case 1: run_wave(std::integral_constant<int, 1>{}); break;
        case 2: run_wave(std::integral_constant<int, 2>{}); break;
        default: run_wave(std::integral_constant<int, 3>{}); break;
    }
#undef DEV_R
#undef DEV_BARRIER
    // ---- the program has ended (its last barrier is behind it): factors and entry words into dead scratch, then the sums
    double* fs = pose_factor_stage(s);
    int32_t* ws = pose_word_stage(s);
    fs[tid] = fac;
#pragma unroll
    for (int it = 0; it < PP_EW; ++it) ws[tid + it * WG] = w[it];
    lds_barrier();
    int bad = 0;
    if constexpr (MODE == PP_LGRAD) {
        if (tid < POSE_NX) {
            const double xb = pose_xbar_column(sig, s.grad[pose_to_knot_col(tid)], dir, ws, fs, s.jac);
            bad = !isfinite(xb);
            pa.out[size_t(b) * POSE_NX + tid] = xb;
        }
    } else {
        const double y = pose_jv_row(dir, ws, fs, s.jac);                                   // (behind m: an empty range, +0.0)
        const double d = tid == PP_DOT_THREAD ? pose_gradf_dot_v(s.grad, fs) : 0.0;
        bad = int(!isfinite(y)) | int(!isfinite(d));
        if (pa.out && tid < m) pa.out[size_t(b) * m + tid] = y;
        if (pa.dot && tid == PP_DOT_THREAD) pa.dot[b] = d;
    }
    const int anybad = pose_vote(tabs, bad, lane);
    if (tid == 0) a.flags[b] = anybad;
}

// Occupancy of hipnlp_pose_kernel, whose program and scratch these are: planar terrain five workgroups per CU, smooth steps four.
template <int TERRAIN> __global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 4, TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 4)))
void hipnlp_pose_lgrad_kernel(PPArgs pa) {
    using Scratch = PoseScratchT<TERRAIN>;
    __shared__ Scratch s;
    __shared__ PoseSharedT<Scratch::trimmed> tabs;
    static_assert(sizeof(Scratch) + sizeof(PoseSharedT<Scratch::trimmed>) <= (TERRAIN == HIPNLP_TERRAIN_PLANAR ? 32000 : 40960), "five / four workgroups per CU");
    pose_first_order<TERRAIN, PP_LGRAD>(pa, s, tabs);
}
template <int TERRAIN> __global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 4, TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 4)))
void hipnlp_pose_jvp_kernel(PPArgs pa) {
    using Scratch = PoseScratchT<TERRAIN>;
    __shared__ Scratch s;
    __shared__ PoseSharedT<Scratch::trimmed> tabs;
    static_assert(sizeof(Scratch) + sizeof(PoseSharedT<Scratch::trimmed>) <= (TERRAIN == HIPNLP_TERRAIN_PLANAR ? 32000 : 40960), "five / four workgroups per CU");
    pose_first_order<TERRAIN, PP_JVP>(pa, s, tabs);
}

// H(x, sigma, lambda) v: what hipnlp_pose_hess_kernel runs — the scratch without grad and jac, hx, the multiplier scatter between the two
// staging barriers, the Hessian program — and then one variable per thread over its touches instead of the copy-out through hperm.
// The touch words, this thread's directory word and its element of v are fetched behind the last barrier but one (in flight across the
// last phase, their registers free before it) and staged over the knot scratch s_raw once the program has ended: every member of it is
// kinematics or a parameter record by then, read by no one; hx (lam, Y, qq, H) is not touched.
constexpr int POSE_HESS_BARRIERS = 6, POSE_HVP_TABLES_AT = POSE_HESS_BARRIERS - 1;
template <int TERRAIN> __global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 3, TERRAIN == HIPNLP_TERRAIN_PLANAR ? 5 : 3)))
void hipnlp_pose_hvp_kernel(PPArgs pa) {
    using Scratch = typename PoseHessEm<TERRAIN>::Scratch;
    constexpr size_t S_WORDS = offsetof(Scratch, grad) / sizeof(double);
    __shared__ alignas(16) double s_raw[S_WORDS];
    Scratch& s = *reinterpret_cast<Scratch*>(s_raw);
    __shared__ PoseSharedT<Scratch::trimmed> tabs;
    __shared__ HessScratch hx;
    constexpr size_t TW_WORDS = PP_TOUCH_CAP * sizeof(int32_t) / sizeof(double);
    static_assert(TW_WORDS + PP_WG <= S_WORDS && POSE_NX <= PP_WG, "touch words and v on the dead knot scratch");
    const PArgs& a = pa.p;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x;
    const PoseTables& tb = *a.tb;
    const PoseProdTables& pt = *pa.pt;
    // (the multipliers: as hipnlp_pose_hess_kernel)
    const int m = a.m;
    double lam_i = 0.0, sig = 0.0;
    int slot_i = -1;
    if (tid < m) { lam_i = a.lambda[size_t(b) * m + tid]; slot_i = tb.row_slot[tid]; }
    if (tid == 0) sig = a.sigma[b];
    for (int slot = tid; slot < gs::COUNT; slot += WG) hx.lam[slot] = 0.0;
    pose_stage(a, s, tabs, b, tid, [&]() { if (slot_i >= 0) hx.lam[slot_i] = lam_i; if (tid == 0) hx.sigma = sig; });

    int32_t w[PP_TW], dir = 0;
    double vi = 0.0;
    auto fetch_tables = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < PP_TW; ++it) w[it] = pt.touch_word[tid + it * WG];
        dir = pt.var_dir[tid];
        if (tid < POSE_NX) vi = pa.v[size_t(b) * POSE_NX + tid];
    };
    int bar = 0;   // barriers passed (the program is straight-line code: a constant at every use)
    KnotInfo ki{1, 3, 0, 0};
    PoseHessEm<TERRAIN> em{nullptr, nullptr, hx.H};   // (no task of the Hessian program emits a row or a Jacobian entry)
    Ctx<PoseHessEm<TERRAIN>> cx(s, tabs.kt, tabs.ks, tabs.gp, ki, em, &tb.head.kt, a.gp + b);
    cx.hands = pose_hands(s, tabs);
    HCtx<PoseHessEm<TERRAIN>> hcx{cx, hx};
#define DEV_KIN(w, fn, nt) if constexpr ((w) == W) { for (int t_ = lane; t_ < (nt); t_ += 64) fn(cx, t_); }
#define DEV_RH(w, fn, nt) if constexpr ((w) == W) { for (int t_ = lane; t_ < (nt); t_ += 64) fn(hcx, t_); }
#define DEV_BARRIER lds_barrier(); if (++bar == POSE_HVP_TABLES_AT) fetch_tables();
    auto run_wave = [&](auto wc) __attribute__((always_inline)) {
        constexpr int W = decltype(wc)::value;
        HIPNLP_POSE_HESS_PROGRAM(DEV_KIN, DEV_RH, DEV_BARRIER)
    };
    switch (wave) {   // (as hipnlp_pose_hess_kernel: the same program instances)
        case 0: run_wave(std::integral_constant<int, 0>{}); break;
        case 1: run_wave(std::integral_constant<int, 1>{}); break;
        case 2: run_wave(std::integral_constant<int, 2>{}); break;
        default: run_wave(std::integral_constant<int, 3>{}); break;
    }
#undef DEV_KIN
#undef DEV_RH
#undef DEV_BARRIER
    // ---- the program has ended (its last barrier is behind it): touch words and v over the dead knot scratch, then one variable per thread
    int32_t* ws = reinterpret_cast<int32_t*>(s_raw);
    double* vs = s_raw + TW_WORDS;
#pragma unroll
    for (int it = 0; it < PP_TW; ++it) ws[tid + it * WG] = w[it];
    vs[tid] = vi;
    lds_barrier();
    int bad = 0;
    if (tid < POSE_NX) {
        const double y = pose_hv_row(dir, ws, vs, hx.H);
        bad = !isfinite(y);
        pa.out[size_t(b) * POSE_NX + tid] = y;
    }
    const int anybad = pose_vote(tabs, bad, lane);
    if (tid == 0) a.flags[b] = anybad;
}

// =====================================================================================================================
// The KKT chain of a pose from STORED value runs (pose_kkt.h has the sums, the element expressions and the order of everything): the
// operator, the diagonal preconditioner and a whole MINRES solve, ONE launch each, one workgroup of 256 threads per pose, no pose program.
// A workgroup stages both value runs by CCS position, the three word tables and a vector record: 31.1 KB of LDS.  Every staging load is
// requested before the first LDS store.  Thread t owns element t of the top (t < 81) and row t of the bottom (t < m).
// =====================================================================================================================
struct PKArgs {
    const PoseKktTables* kt;
    const PoseProdTables* pt;     // (its three directories)
    const double* hess;           // [batch][hnnz]
    const double* jac;            // [batch][nnz]
    const double* dx;             // [batch][81]  or null
    const double* dc;             // [batch][m]   or null
    const double* in_top;         // [batch][81]  v (times), rhs_top (solve)
    const double* in_bot;         // [batch][m]   w (times), rhs_bottom (solve)
    const double* minv_top;       // [batch][81]  or null (solve: the caller's preconditioner)
    const double* minv_bot;       // [batch][m]   or null
    double* out_top;              // [batch][81]  top (times), minv_top (diag), sol_top (solve)
    double* out_bot;              // [batch][m]
    int32_t* iterations;          // [batch]      solve only
    double* residual;             // [batch]
    int32_t* status;              // [batch]
    double floor, rtol;
    int32_t maxit, build_diag, m, nnz, hnnz;
};

struct alignas(16) PoseKktLds {
    double jac[PP_ENT_CAP];
    double hess[PK_HESS_CAP];
    int32_t cw[PP_ENT_CAP], rw[PP_ENT_CAP], tw[PP_TOUCH_CAP];
    double vec[PK_VEC_WORDS];     // the vector record of the operator; minv_top while the diagonal is built
    double part[2][4];            // the wave sums of the two trees of an iteration (pose_kkt_tree)
};
static_assert(sizeof(PoseKktLds) <= 32000, "five workgroups per CU by LDS (25 granules of 1 280 B)");
static_assert(PK_WG == WG && PP_ENT_CAP % WG == 0 && PK_HESS_CAP % WG == 0 && PP_TOUCH_CAP % WG == 0, "staged by 256 threads");

// the staging loads of one thread: issue() requests them all, land() writes them to LDS (no barrier here)
struct PoseKktStage {
    static constexpr int JB = PP_ENT_CAP / WG, HB = PK_HESS_CAP / WG, TB = PP_TOUCH_CAP / WG;
    double j[JB], h[HB];
    int32_t c[JB], r[JB], t[TB];
    int32_t col_dir, row_dir, var_dir;
    template <bool OPERATOR> __device__ __forceinline__ void issue(const PKArgs& a, int b, int tid) {
        const double* jv = a.jac + size_t(b) * size_t(a.nnz);
#pragma unroll
        for (int it = 0; it < JB; ++it) { const int i = tid + it * WG; j[it] = i < a.nnz ? jv[i] : 0.0; }
#pragma unroll
        for (int it = 0; it < JB; ++it) r[it] = a.kt->row_word[tid + it * WG];
        row_dir = a.pt->row_dir[tid];
        if constexpr (OPERATOR) {
            const double* hv = a.hess + size_t(b) * size_t(a.hnnz);
#pragma unroll
            for (int it = 0; it < HB; ++it) { const int i = tid + it * WG; h[it] = i < a.hnnz ? hv[i] : 0.0; }
#pragma unroll
            for (int it = 0; it < JB; ++it) c[it] = a.kt->col_word[tid + it * WG];
#pragma unroll
            for (int it = 0; it < TB; ++it) t[it] = a.kt->touch_word[tid + it * WG];
            col_dir = a.pt->col_dir[tid];
            var_dir = a.pt->var_dir[tid];
        }
    }
    template <bool OPERATOR> __device__ __forceinline__ void land(PoseKktLds& s, int tid) const {
#pragma unroll
        for (int it = 0; it < JB; ++it) { s.jac[tid + it * WG] = j[it]; s.rw[tid + it * WG] = r[it]; }
        if constexpr (OPERATOR) {
#pragma unroll
            for (int it = 0; it < HB; ++it) s.hess[tid + it * WG] = h[it];
#pragma unroll
            for (int it = 0; it < JB; ++it) s.cw[tid + it * WG] = c[it];
#pragma unroll
            for (int it = 0; it < TB; ++it) s.tw[tid + it * WG] = t[it];
        }
    }
};

// The tree of jprod_dot_tree over the workgroup's 256 per-thread chains: a butterfly over the lanes, then the four waves in order; every
// thread returns the sum.  part: four words of LDS.  The solve calls it twice per iteration and gives the two calls DIFFERENT words
// (PoseKktLds::part[0] and [1]): nothing separates the reads of one tree from the stores of the next tree, but between two uses of the
// same four words lies the barrier of the other tree — no barrier of its own is needed.
__device__ __forceinline__ double pose_kkt_tree(double acc, double* part) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, s, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    lds_barrier();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

// minv_top of this thread's variable and minv_bottom of its row (pose_kkt.h); minv_top goes through s.vec.  Ends with a barrier: s.vec is free.
__device__ __forceinline__ void pose_kkt_diagonal(PoseKktLds& s, const PoseKktStaged& st, int tid, int m, int32_t row_dir, bool with_dx, double dx_c, bool with_dc, double dc_i,
                                                  double h_cc, double floor, double& mt, double& mb) {
    mt = tid < POSE_NX ? pose_kkt_minv_top(with_dx, h_cc, dx_c, floor) : 0.0;
    if (tid < PK_BOT) s.vec[tid] = mt;
    lds_barrier();
    mb = tid < m ? pose_kkt_minv_bottom(st, row_dir, s.vec, with_dc, dc_i, floor) : 0.0;
    lds_barrier();
}

__global__ __launch_bounds__(WG) void hipnlp_pose_saddle_times_kernel(PKArgs a) {
    __shared__ PoseKktLds s;
    const int tid = threadIdx.x, b = blockIdx.x, m = a.m;
    const bool has_top = tid < POSE_NX, has_row = tid < m;
    PoseKktStage stage;
    stage.issue<true>(a, b, tid);
    const double v = has_top ? a.in_top[size_t(b) * POSE_NX + tid] : 0.0;
    const double w = has_row ? a.in_bot[size_t(b) * m + tid] : 0.0;
    const double dx = (a.dx && has_top) ? a.dx[size_t(b) * POSE_NX + tid] : 0.0;
    const double dc = (a.dc && has_row) ? a.dc[size_t(b) * m + tid] : 0.0;
    stage.land<true>(s, tid);
    if (tid < PK_BOT) s.vec[tid] = v;
    s.vec[PK_BOT + tid] = w;
    lds_barrier();
    const PoseKktStaged st{s.jac, s.hess, s.cw, s.rw, s.tw};
    if (has_top) a.out_top[size_t(b) * POSE_NX + tid] = pose_kkt_top(st, stage.var_dir, stage.col_dir, s.vec, a.dx != nullptr, dx, v);
    if (has_row) a.out_bot[size_t(b) * m + tid] = pose_kkt_bottom(st, stage.row_dir, s.vec, a.dc != nullptr, dc, w);
}

__global__ __launch_bounds__(WG) void hipnlp_pose_saddle_diag_kernel(PKArgs a) {
    __shared__ PoseKktLds s;
    const int tid = threadIdx.x, b = blockIdx.x, m = a.m;
    const bool has_top = tid < POSE_NX, has_row = tid < m;
    PoseKktStage stage;
    stage.issue<false>(a, b, tid);
    const int32_t hd = a.kt->hdiag[tid];
    const double dx = (a.dx && has_top) ? a.dx[size_t(b) * POSE_NX + tid] : 0.0;
    const double dc = (a.dc && has_row) ? a.dc[size_t(b) * m + tid] : 0.0;
    const double h_cc = (has_top && hd >= 0) ? a.hess[size_t(b) * size_t(a.hnnz) + hd] : 0.0;   // (addressed by a table word: the one load that waits for another)
    stage.land<false>(s, tid);
    lds_barrier();
    const PoseKktStaged st{s.jac, s.hess, s.cw, s.rw, s.tw};
    double mt, mb;
    pose_kkt_diagonal(s, st, tid, m, stage.row_dir, a.dx != nullptr, dx, a.dc != nullptr, dc, h_cc, a.floor, mt, mb);
    if (has_top) a.out_top[size_t(b) * POSE_NX + tid] = mt;
    if (has_row) a.out_bot[size_t(b) * m + tid] = mb;
}

// The whole solve of a pose: the start, then iterations until the pose has a status — the scalars (MinresRec) are computed by every thread
// from the same LDS words, so the loop exit is the same in every thread and every wave meets every barrier.  Per iteration: one barrier
// behind the stores of v, one in each of the two trees.  Nothing is stored to memory before the loop has ended.
__global__ __launch_bounds__(WG) void hipnlp_pose_saddle_solve_kernel(PKArgs a) {
    __shared__ PoseKktLds s;
    const int tid = threadIdx.x, b = blockIdx.x, m = a.m;
    const bool has_top = tid < POSE_NX, has_row = tid < m;
    PoseKktStage stage;
    stage.issue<true>(a, b, tid);
    const int32_t hd = a.build_diag ? a.kt->hdiag[tid] : -1;
    const double bt = has_top ? a.in_top[size_t(b) * POSE_NX + tid] : 0.0;
    const double bb = has_row ? a.in_bot[size_t(b) * m + tid] : 0.0;
    const bool with_dx = a.dx != nullptr, with_dc = a.dc != nullptr;
    const double dx = (with_dx && has_top) ? a.dx[size_t(b) * POSE_NX + tid] : 0.0;
    const double dc = (with_dc && has_row) ? a.dc[size_t(b) * m + tid] : 0.0;
    bool with_minv = a.minv_top != nullptr;
    double mt = (with_minv && has_top) ? a.minv_top[size_t(b) * POSE_NX + tid] : 0.0;
    double mb = (with_minv && has_row) ? a.minv_bot[size_t(b) * m + tid] : 0.0;
    stage.land<true>(s, tid);
    lds_barrier();
    const PoseKktStaged st{s.jac, s.hess, s.cw, s.rw, s.tw};
    if (a.build_diag) {   // (a kernel argument: the same in every thread)
        pose_kkt_diagonal(s, st, tid, m, stage.row_dir, with_dx, dx, with_dc, dc, (has_top && hd >= 0) ? s.hess[hd] : 0.0, a.floor, mt, mb);
        with_minv = true;
    }
    PoseKktElem et, eb;
    pose_kkt_elem_start(et, bt, with_minv, mt);
    pose_kkt_elem_start(eb, bb, with_minv, mb);
    MinresRec rec = minres_init(pose_kkt_tree(pose_kkt_chain(has_top, et.r2, et.y, has_row, eb.r2, eb.y), s.part[1]), a.rtol, a.maxit);
    while (__builtin_amdgcn_readfirstlane(rec.status) == MINRES_RUNNING) {
        pose_kkt_elem_v(et, rec.beta);
        pose_kkt_elem_v(eb, rec.beta);
        if (has_top) s.vec[tid] = et.v;
        if (has_row) s.vec[PK_BOT + tid] = eb.v;
        lds_barrier();
        const bool sub = rec.it >= 1;
        const double c1 = sub ? minres_div(rec.beta, rec.oldb) : 0.0;
        const double kt = has_top ? pose_kkt_top(st, stage.var_dir, stage.col_dir, s.vec, with_dx, dx, et.v) : 0.0;
        const double kb = has_row ? pose_kkt_bottom(st, stage.row_dir, s.vec, with_dc, dc, eb.v) : 0.0;
        pose_kkt_elem_apply(et, sub, c1, kt);
        pose_kkt_elem_apply(eb, sub, c1, kb);
        const double alfa = pose_kkt_tree(pose_kkt_chain(has_top, et.v, et.y, has_row, eb.v, eb.y), s.part[0]);
        const double c2 = minres_div(alfa, rec.beta);
        pose_kkt_elem_residual(et, c2, with_minv);
        pose_kkt_elem_residual(eb, c2, with_minv);
        const double sum = pose_kkt_tree(pose_kkt_chain(has_top, et.r2, et.y, has_row, eb.r2, eb.y), s.part[1]);
        MinresStep step;
        const MinresRec next = minres_step(rec, alfa, sum, a.rtol, a.maxit, step);
        if (next.status != MINRES_BREAKDOWN) {   // (a breakdown leaves z as it was)
            pose_kkt_elem_update(et, step);
            pose_kkt_elem_update(eb, step);
        }
        rec = next;
    }
    if (has_top) a.out_top[size_t(b) * POSE_NX + tid] = et.z;
    if (has_row) a.out_bot[size_t(b) * m + tid] = eb.z;
    if (tid == 0) { a.iterations[b] = rec.it; a.residual[b] = rec.residual; a.status[b] = rec.status; }
}

// =====================================================================================================================
// The dense L D L^T of the KKT matrix of a pose (pose_ldl.h has the element expressions, the choice of the pivot and the order of
// everything): ONE workgroup per pose holds the packed lower triangle, order 81 + m <= 176, in 127 KB of static LDS — one workgroup
// per CU — and assembles it from the two stored value runs, factors it with Bunch-Kaufman pivoting, counts the inertia, climbs the
// regularisation ladder and solves, all in one launch.  Nothing leaves the CU, no workgroup waits for another, every loop is bounded.
//
// 1 024 threads (chosen by reading, 256 and 512 UNMEASURED; DESIGN.md "Pose LDL"; timings profiles/r15_pose_ldl.txt): the trailing update is bound by LDS traffic (a read of x_i, a read and a store of
// a_ij per fused multiply-add), one workgroup has the CU to itself, and sixteen waves — four per SIMD — keep that many LDS requests in
// flight without unrolling; the price is a dearer barrier, four per pivot step.
//   search   EVERY wave searches column k (and, where the diagonal does not stand, row / column imax) itself: the same LDS words,
//            pl_max_join over its lanes — the same result in every wave, no barrier, no exchange; lanes along the column.
//   B1       every wave has read what it searched
//   swap     thread t owns the one pair of index t that the interchange kk <-> kp moves (B2 behind it, only where there is one)
//   column   thread t forms the multipliers of row k + kstep + t, keeps the entry before the scaling in x0 / x1 (B3)
//   update   columns dealt to the waves, lanes along the packed column: unit stride, no (i, j) from a linear index (B4)
// The solves: one WAVE per right-hand side, the vector in three registers per lane, y_k by a lane broadcast: no LDS for the vector, no
// barrier.  The backward pass reads a row of L (a stride that grows lane by lane).
// =====================================================================================================================
constexpr int LDL_WG = 1024, LDL_WAVES = LDL_WG / 64;
static_assert(PL_MAX_N <= 3 * 64 && PL_MAX_NRHS <= LDL_WAVES && PL_MAX_N <= LDL_WG - 128, "a solve is one wave with three elements per lane; one thread per index");

struct PLArgs {
    const PoseLdlTables* lt;
    const double* hess;           // [batch][hnnz]
    const double* jac;            // [batch][nnz]
    const double* dx;             // [batch][81]  or null
    const double* dc;             // [batch][m]   or null
    const double* rhs_top;        // [batch][nrhs][81]
    const double* rhs_bot;        // [batch][nrhs][m]
    double* sol_top;
    double* sol_bot;
    int32_t* inertia;             // [batch][3]
    int32_t* status;              // [batch]
    double* delta;                // [batch] or null
    int32_t* tries;               // [batch] or null
    double* factor;               // [batch][N (N + 1) / 2] or null: a destination of the factorisation, the source of the stored-factor solve
    int32_t* pivots;              // [batch][N]
    double delta_init, kappa;
    int32_t max_tries, nrhs, m, nnz, hnnz;
};

struct alignas(16) PoseLdlLds {
    double a[PL_MAX_DOUBLES];     // the packed lower triangle: K, then L and D in place
    double x0[PL_MAX_N], x1[PL_MAX_N];   // the pivot column(s) before the scaling
    int32_t ipiv[PL_MAX_N], perm[PL_MAX_N], kind[PL_MAX_N];   // the pivot vector; b~_i = b_perm[i]; PL_ONE / PL_FIRST / PL_SECOND
    int32_t word[4];              // inertia and status, for the exit of the ladder
};
static_assert(sizeof(PoseLdlLds) <= 160 * 1024, "one workgroup per CU");

__device__ __forceinline__ PlMax pose_ldl_wave_max(PlMax a) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) a = pl_max_join(a, PlMax{__shfl_xor(a.v, o, 64), __shfl_xor(a.at, o, 64), __shfl_xor(a.bad, o, 64)});
    return a;
}

// K of one try into s.a.  Ends with a barrier.
__device__ __forceinline__ void pose_ldl_assemble(PoseLdlLds& s, const PLArgs& a, int b, int N, int tid, bool with_dx, double dx_c, bool with_dc, double dc_i, bool with_delta,
                                                  double delta) {
    const int nd = pl_doubles(N);
    for (int e = tid; e < nd; e += LDL_WG) s.a[e] = 0.0;
    lds_barrier();
    const double* hv = a.hess + size_t(b) * size_t(a.hnnz);
    const double* jv = a.jac + size_t(b) * size_t(a.nnz);
    for (int e = tid; e < a.hnnz; e += LDL_WG) s.a[a.lt->hess_at[e]] = hv[e];
    for (int e = tid; e < a.nnz; e += LDL_WG) s.a[a.lt->jac_at[e]] = jv[e];
    lds_barrier();
    if (tid < POSE_NX) { const int p = pl_col(N, tid); s.a[p] = pl_diag_top(s.a[p], with_dx, dx_c, with_delta, delta); }
    else if (tid >= 128 && tid - 128 < a.m) s.a[pl_col(N, POSE_NX + tid - 128)] = pl_diag_bottom(with_dc, dc_i);
    lds_barrier();
}

// The factorisation of s.a in place; the status of this try.  Every thread takes every branch the same way: what it branches on comes
// from LDS words that no thread writes between the barrier in front of the search and B1.  The caller puts a barrier behind it.
__device__ __forceinline__ int pose_ldl_factor(PoseLdlLds& s, int N, int tid, int& pos, int& neg, int& zero) {
    const int lane = tid & 63, wave = tid >> 6;
    pos = neg = zero = 0;
    if (tid < N) s.perm[tid] = tid;
    int k = 0;
    while (k < N) {
        const int kc = pl_col(N, k);
        const double akk = s.a[kc];
        PlMax cm = pl_max_none();
        for (int i = k + 1 + lane; i < N; i += 64) cm = pl_max_join(cm, pl_max_of(s.a[kc + i - k], i));
        cm = pose_ldl_wave_max(cm);
        int bad = cm.bad | (minres_finite(akk) ? 0 : 1);
        const double absakk = pl_abs(akk), colmax = cm.v < 0.0 ? 0.0 : cm.v;
        int kp = k, kstep = 1;
        double arr = 0.0;
        bool zero_column = false;
        if (!bad) {
            if (pl_column_is_zero(absakk, colmax)) zero_column = true;
            else if (!pl_keep_diagonal(absakk, colmax)) {
                const int imax = cm.at, pc = pl_col(N, imax);
                PlMax rm = pl_max_none();
                for (int j = k + lane; j < imax; j += 64) rm = pl_max_join(rm, pl_max_of(s.a[pl_at(N, imax, j)], j));
                for (int i = imax + 1 + lane; i < N; i += 64) rm = pl_max_join(rm, pl_max_of(s.a[pc + i - imax], i));
                rm = pose_ldl_wave_max(rm);
                arr = s.a[pc];
                bad = rm.bad | (minres_finite(arr) ? 0 : 1);
                if (!bad) { const PlPivot pv = pl_choose(k, imax, absakk, colmax, rm.v, pl_abs(arr)); kp = pv.kp; kstep = pv.kstep; }
            }
        }
        if (__builtin_amdgcn_readfirstlane(bad | int(zero_column))) {
            if (tid >= k && tid < N) { s.ipiv[tid] = tid + 1; s.kind[tid] = PL_ONE; }
            if (bad) return PL_NONFINITE;
            zero = 1;
            return PL_SINGULAR;
        }
        kp = __builtin_amdgcn_readfirstlane(kp);
        kstep = __builtin_amdgcn_readfirstlane(kstep);
        const int kk = k + kstep - 1, knc = pl_col(N, kk), base = k + kstep;
        lds_barrier();                                                        // B1
        if (kp != kk) {
            if (tid < N && tid != kp) {
                const int pcol = pl_col(N, kp);
                int p, q;
                if (tid < kk) { p = pl_at(N, kk, tid); q = pl_at(N, kp, tid); }          // the rows kk and kp of a column in front (and, of a 2x2 pivot, of column k)
                else if (tid == kk) { p = knc; q = pcol; }                               // the two diagonal elements
                else if (tid < kp) { p = knc + tid - kk; q = pl_at(N, kp, tid); }        // column kk between them against row kp
                else { p = knc + tid - kk; q = pcol + tid - kp; }                        // the two columns below kp
                const double u = s.a[p];
                s.a[p] = s.a[q];
                s.a[q] = u;
            } else if (tid == kp) {
                const int32_t u = s.perm[kk];
                s.perm[kk] = s.perm[kp];
                s.perm[kp] = u;
            }
            lds_barrier();                                                    // B2
        }
        if (kstep == 1) {
            const double d = kp == k ? akk : arr;
            if (d > 0.0) ++pos; else ++neg;
            if (tid == 0) { s.ipiv[k] = kp + 1; s.kind[k] = PL_ONE; }
            const int i = base + tid;
            if (i < N) { const double x = s.a[kc + i - k]; s.x0[i] = x; s.a[kc + i - k] = pl_l1(x, d); }
        } else {
            ++pos; ++neg;
            if (tid == 0) { s.ipiv[k] = s.ipiv[k + 1] = -(kp + 1); s.kind[k] = PL_FIRST; s.kind[k + 1] = PL_SECOND; }
            const PlBlock blk = pl_block(s.a[kc], s.a[kc + 1], s.a[knc]);
            const int i = base + tid;
            if (i < N) {
                const double x0 = s.a[kc + i - k], x1 = s.a[knc + i - kk];
                s.x0[i] = x0; s.x1[i] = x1;
                s.a[kc + i - k] = pl_w_first(blk, x0, x1);
                s.a[knc + i - kk] = pl_w_second(blk, x0, x1);
            }
        }
        lds_barrier();                                                        // B3
        for (int j = base + wave; j < N; j += LDL_WAVES) {
            const int cj = pl_col(N, j) - j;                                  // (i, j) at cj + i
            if (kstep == 1) {
                const double lj = s.a[kc + j - k];
                for (int i = j + lane; i < N; i += 64) s.a[cj + i] = pl_update1(s.a[cj + i], s.x0[i], lj);
            } else {
                const double w0 = s.a[kc + j - k], w1 = s.a[knc + j - kk];
                for (int i = j + lane; i < N; i += 64) s.a[cj + i] = pl_update2(s.a[cj + i], s.x0[i], s.x1[i], w0, w1);
            }
        }
        lds_barrier();                                                        // B4
        k = base;
    }
    return PL_OK;
}

// One right-hand side by one wave: lane l holds the elements l, l + 64, l + 128 of the vector in three named registers (no array: nothing
// for the compiler to put into scratch memory or LDS).  good: the factor can be solved with; else the solution is NaN.  bt, bb, xt, xb: of
// this pose and this right-hand side.  LDL_ROWS(F) states F(r, y_r, src_r) for the three elements of a lane.
#define LDL_ROWS(F) F(0, y0, src0) F(1, y1, src1) F(2, y2, src2)
__device__ __forceinline__ void pose_ldl_solve_wave(const PoseLdlLds& s, int N, bool good, const double* bt, const double* bb, double* xt, double* xb, int lane) {
    double y0, y1, y2;
    int src0, src1, src2;
#define LDL_LOAD(r, y, src)                                                                         \
    src = (lane + 64 * r) < N ? s.perm[lane + 64 * r] : -1;                                         \
    y = (src >= 0 && good) ? (src < POSE_NX ? bt[src] : bb[src - POSE_NX]) : 0.0;
    LDL_ROWS(LDL_LOAD)
#undef LDL_LOAD
    if (good) {
        for (int k = 0; k < N; ++k) {                                          // forward: column k of L, (i, k) at c + i
            const int lo = k + 1 + (s.kind[k] == PL_FIRST ? 1 : 0), c = pl_col(N, k) - k, kr = k >> 6;
            const double yk = __shfl(kr == 0 ? y0 : (kr == 1 ? y1 : y2), k & 63, 64);
#define LDL_FORWARD(r, y, src) { const int i = lane + 64 * r; if (i >= lo && i < N) y = pl_axpy(y, s.a[c + i], yk); }
            LDL_ROWS(LDL_FORWARD)
#undef LDL_FORWARD
        }
        // the diagonal: element i needs i + 1 (the first of a 2x2 block) or i - 1 (the second), all taken before any is changed
        const int nl = (lane + 1) & 63, pl = (lane + 63) & 63;
        const double n0 = __shfl(y0, nl, 64), n1 = __shfl(y1, nl, 64), n2 = __shfl(y2, nl, 64);
        const double p0 = __shfl(y0, pl, 64), p1 = __shfl(y1, pl, 64), p2 = __shfl(y2, pl, 64);
        const double up0 = lane == 63 ? n1 : n0, up1 = lane == 63 ? n2 : n1, up2 = n2;          // (lane 63's next element is lane 0's of the next register)
        const double dn0 = p0, dn1 = lane == 0 ? p0 : p1, dn2 = lane == 0 ? p1 : p2;
#define LDL_DIAGONAL(r, y, src)                                                                                                              \
        {                                                                                                                                    \
            const int i = lane + 64 * r;                                                                                                     \
            if (i < N) {                                                                                                                     \
                const int kd = s.kind[i], ci = pl_col(N, i);                                                                                 \
                if (kd == PL_ONE) y = pl_diag1(y, s.a[ci]);                                                                                  \
                else if (kd == PL_FIRST) y = pl_diag2_first(pl_solve_block(s.a[ci], s.a[ci + 1], s.a[pl_col(N, i + 1)]), y, up##r);          \
                else y = pl_diag2_second(pl_solve_block(s.a[pl_col(N, i - 1)], s.a[pl_col(N, i - 1) + 1], s.a[ci]), dn##r, y);               \
            }                                                                                                                                \
        }
        LDL_ROWS(LDL_DIAGONAL)
#undef LDL_DIAGONAL
        const int rb0 = pl_col(N, lane) - lane, rb1 = pl_col(N, lane + 64) - (lane + 64), rb2 = pl_col(N, lane + 128) - (lane + 128);   // (i, k) at rb_k + i
        for (int i = N - 1; i >= 0; --i) {                                     // backward: row i of L
            const int hi = i - 1 - (s.kind[i] == PL_SECOND ? 1 : 0), ir = i >> 6;
            const double yi = __shfl(ir == 0 ? y0 : (ir == 1 ? y1 : y2), i & 63, 64);
#define LDL_BACKWARD(r, y, src) { if (lane + 64 * r <= hi) y = pl_axpy(y, s.a[rb##r + i], yi); }
            LDL_ROWS(LDL_BACKWARD)
#undef LDL_BACKWARD
        }
    }
#define LDL_STORE(r, y, src)                                                                        \
    if (src >= 0) {                                                                                 \
        const double v = good ? y : pl_nan();                                                       \
        if (src < POSE_NX) xt[src] = v; else xb[src - POSE_NX] = v;                                 \
    }
    LDL_ROWS(LDL_STORE)
#undef LDL_STORE
}
#undef LDL_ROWS

__global__ __launch_bounds__(LDL_WG) void hipnlp_pose_saddle_ldl_kernel(PLArgs a) {
    __shared__ PoseLdlLds s;
    const int tid = threadIdx.x, b = blockIdx.x, m = a.m, N = POSE_NX + m;
    const bool with_dx = a.dx != nullptr, with_dc = a.dc != nullptr;
    const double dx_c = (with_dx && tid < POSE_NX) ? a.dx[size_t(b) * POSE_NX + tid] : 0.0;
    const double dc_i = (with_dc && tid >= 128 && tid - 128 < m) ? a.dc[size_t(b) * m + (tid - 128)] : 0.0;
    double delta = 0.0;
    int t = 0, status, pos, neg, zero;
    for (;;) {                                                                 // the ladder: at most max_tries + 1 <= 17 turns
        pose_ldl_assemble(s, a, b, N, tid, with_dx, dx_c, with_dc, dc_i, t > 0, delta);
        const int st = pose_ldl_factor(s, N, tid, pos, neg, zero);
        if (tid == 0) { s.word[0] = pos; s.word[1] = neg; s.word[2] = zero; s.word[3] = st; }
        lds_barrier();
        pos = s.word[0]; neg = s.word[1]; zero = s.word[2];                    // the same words in every thread: the exit is the workgroup's
        const bool wanted = pl_inertia_wanted(pos, neg, zero, m);
        status = pl_final_status(s.word[3], wanted, a.max_tries);
        if (!__builtin_amdgcn_readfirstlane(int(pl_ladder_goes_on(s.word[3], wanted, t, a.max_tries)))) break;
        ++t;
        delta = pl_next_delta(t, delta, a.delta_init, a.kappa);
    }
    if (tid == 0) {
        a.inertia[size_t(b) * 3 + 0] = pos; a.inertia[size_t(b) * 3 + 1] = neg; a.inertia[size_t(b) * 3 + 2] = zero;
        a.status[b] = status;
        if (a.delta) a.delta[b] = delta;
        if (a.tries) a.tries[b] = t;
    }
    if (a.factor) {
        const int nd = pl_doubles(N);
        double* f = a.factor + size_t(b) * size_t(nd);
        for (int e = tid; e < nd; e += LDL_WG) f[e] = s.a[e];
        if (tid < N) a.pivots[size_t(b) * N + tid] = s.ipiv[tid];
    }
    const int wave = tid >> 6;
    if (wave < a.nrhs) {
        const size_t r = size_t(b) * size_t(a.nrhs) + size_t(wave);
        pose_ldl_solve_wave(s, N, status == PL_OK || status == PL_EXHAUSTED, a.rhs_top + r * POSE_NX, a.rhs_bot + r * m, a.sol_top + r * POSE_NX, a.sol_bot + r * m, tid & 63);
    }
}

// nrhs solves from a stored factor and pivot vector: no assembly, no value run.  A pivot word that names no index of the trailing
// matrix interchanges nothing (the words are the caller's memory: nothing is addressed by them unchecked).
__global__ __launch_bounds__(LDL_WG) void hipnlp_pose_saddle_ldl_solve_kernel(PLArgs a) {
    __shared__ PoseLdlLds s;
    const int tid = threadIdx.x, b = blockIdx.x, m = a.m, N = POSE_NX + m, nd = pl_doubles(N);
    const double* f = a.factor + size_t(b) * size_t(nd);
    if (tid < N) { s.ipiv[tid] = a.pivots[size_t(b) * N + tid]; s.perm[tid] = tid; s.kind[tid] = PL_ONE; }
    for (int e = tid; e < nd; e += LDL_WG) s.a[e] = f[e];
    lds_barrier();
    if (tid == 0) {
        int k = 0;
        while (k < N) {
            const int p = s.ipiv[k];
            const bool two = p < 0 && k + 1 < N;
            const int kk = two ? k + 1 : k;
            int kp = (p < 0 ? -p : p) - 1;
            if (kp < kk || kp >= N) kp = kk;
            if (two) { s.kind[k] = PL_FIRST; s.kind[k + 1] = PL_SECOND; }
            const int32_t u = s.perm[kk];
            s.perm[kk] = s.perm[kp];
            s.perm[kp] = u;
            k = kk + 1;
        }
    }
    lds_barrier();
    const int wave = tid >> 6;
    if (wave < a.nrhs) {
        const size_t r = size_t(b) * size_t(a.nrhs) + size_t(wave);
        pose_ldl_solve_wave(s, N, true, a.rhs_top + r * POSE_NX, a.rhs_bot + r * m, a.sol_top + r * POSE_NX, a.sol_bot + r * m, tid & 63);
    }
}

thread_local std::string g_pose_create_error;

}  // namespace

struct hipnlp_pose_handle {
    hipnlp_pose_desc d;
    PoseLayout L;
    KinTables kt;
    int batch = 1, dev = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing_valid = false, params_set = false, have_result = false;
    bool time_host = false;   // hipnlp_pose_set_host_timing: the host-buffer calls bracket their launch with events (each record drains the stream: ~3 us of a 25 us call)
    PoseTables* d_tb = nullptr;
    PoseProdTables* d_pt = nullptr;   // tables of the product kernels (pose_products.h): a block of their own, PoseTables is what it was
    PoseKktTables* d_kt = nullptr;    // tables of the KKT kernels (pose_kkt.h): a third block, the other two are what they were
    bool kkt_fits = false;            // the pattern is within what the KKT kernels stage (PoseLayout::kkt_fits)
    std::string kkt_error;
    PoseLdlTables* d_lt = nullptr;    // table of the dense factorisation (pose_ldl.h): a fourth block
    bool ldl_fits = false;            // the KKT matrix is within what one workgroup holds (PoseLayout::ldl_fits)
    std::string ldl_error;
    double *d_x = nullptr, *d_pk = nullptr, *d_xr = nullptr, *d_f = nullptr, *d_grad = nullptr, *d_g = nullptr, *d_jac = nullptr, *d_cost = nullptr;
    GParams* d_gp = nullptr;
    int32_t* d_flags = nullptr;
    double *h_x = nullptr, *h_f = nullptr, *h_grad = nullptr, *h_g = nullptr, *h_jac = nullptr, *h_cost = nullptr;
    // host-buffer path: the kernel reads x straight out of the pinned staging copy and stores its outputs straight into the pinned
    // blocks (device-visible addresses of the same memory: no copy command on either side of the launch, as in hipnlp_eval)
    double *hd_x = nullptr, *hd_f = nullptr, *hd_grad = nullptr, *hd_g = nullptr, *hd_jac = nullptr, *hd_cost = nullptr;
    int32_t* hd_flags = nullptr;
    double *hd_sigma = nullptr, *hd_lambda = nullptr, *hd_hess = nullptr;
    int32_t* h_flags = nullptr;
    // Hessian path (allocated on first use)
    double *d_sigma = nullptr, *d_lambda = nullptr, *d_hess = nullptr, *h_sigma = nullptr, *h_lambda = nullptr, *h_hess = nullptr;
    std::vector<double> p;
    std::string err;
#ifdef HIPNLP_STAMPS
    unsigned long long* d_stamps = nullptr;   // diagnostic build only
#endif
};

#define HIP_TRY(h, call)                                                                            \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
            (void)hipGetLastError();                                                                \
            return HIPNLP_E_NODEVICE;                                                               \
        }                                                                                           \
    } while (0)

static void pose_free_all(hipnlp_pose_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->dev);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    void* dptrs[] = {h->d_tb, h->d_pt, h->d_kt, h->d_lt, h->d_x, h->d_pk, h->d_xr, h->d_f, h->d_grad, h->d_g, h->d_jac, h->d_cost, h->d_gp, h->d_flags, h->d_sigma, h->d_lambda, h->d_hess};
    for (void* q : dptrs) if (q) (void)hipFree(q);
    void* hptrs[] = {h->h_x, h->h_f, h->h_grad, h->h_g, h->h_jac, h->h_cost, h->h_flags, h->h_sigma, h->h_lambda, h->h_hess};
    for (void* q : hptrs) if (q) (void)hipHostFree(q);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

static int pose_launch(hipnlp_pose_handle* h, const double* x_dev, double* f_dev, double* grad_dev, double* g_dev, double* jac_dev, hipStream_t s,
                       bool timed, bool host_block = false) {
    PArgs a{};
    a.tb = h->d_tb; a.x = x_dev; a.pk = h->d_pk; a.xr = h->d_xr; a.gp = h->d_gp;
    a.f = f_dev; a.grad = grad_dev; a.g = g_dev; a.jac = jac_dev;
    a.cost_terms = host_block ? h->hd_cost : h->d_cost; a.flags = host_block ? h->hd_flags : h->d_flags;
#ifdef HIPNLP_STAMPS
    if (!h->d_stamps) { HIP_TRY(h, hipMalloc(&h->d_stamps, size_t(h->batch) * 256 * sizeof(unsigned long long))); HIP_TRY(h, hipMemset(h->d_stamps, 0, size_t(h->batch) * 256 * sizeof(unsigned long long))); }
    a.stamps = h->d_stamps;
#endif
    if (timed) HIP_TRY(h, hipEventRecord(h->ev0, s));   // host-buffer path only (an event record drains the stream)
    if (h->d.settings.terrain == HIPNLP_TERRAIN_PLANAR)
        hipLaunchKernelGGL(hipnlp_pose_kernel<HIPNLP_TERRAIN_PLANAR>, dim3(unsigned(h->batch)), dim3(WG), 0, s, a);
    else
        hipLaunchKernelGGL(hipnlp_pose_kernel<HIPNLP_TERRAIN_SMOOTH_STEPS>, dim3(unsigned(h->batch)), dim3(WG), 0, s, a);
    if (timed) HIP_TRY(h, hipEventRecord(h->ev1, s));
    HIP_TRY(h, hipGetLastError());
    if (timed) h->timing_valid = true;
    return HIPNLP_OK;
}

extern "C" {

const char* hipnlp_pose_last_error(const hipnlp_pose_handle* h) { return h ? h->err.c_str() : g_pose_create_error.c_str(); }

int hipnlp_pose_create(const hipnlp_pose_desc* desc, hipnlp_pose_handle** out) {
    if (!desc || !out) { g_pose_create_error = "null argument"; return HIPNLP_E_INVALID; }
    *out = nullptr;
    hipnlp_pose_handle* h = new (std::nothrow) hipnlp_pose_handle();
    if (!h) { g_pose_create_error = "out of memory"; return HIPNLP_E_ALLOC; }
    h->d = *desc;
    const hipnlp_pose_settings& st = desc->settings;
    auto fail = [&](int code, const std::string& msg) { g_pose_create_error = msg; pose_free_all(h); return code; };
    if (desc->abi_version != HIPNLP_ABI_VERSION)
        return fail(HIPNLP_E_INVALID, "hipnlp_pose_desc.abi_version is " + std::to_string(desc->abi_version) + ", this library implements HIPNLP_ABI_VERSION " +
                                          std::to_string(HIPNLP_ABI_VERSION) + " (the caller was built against another include/hipnlp.h, or left the field unset)");
    if (desc->flags != 0) return fail(HIPNLP_E_INVALID, "unknown bits in hipnlp_pose_desc.flags");
    if (const char* te = Layout::check_terrain(st.terrain, st.n_terrain_steps, st.terrain_steps)) return fail(HIPNLP_E_INVALID, te);
    for (int t : {st.com_position_type, st.left_point_position_type, st.right_point_position_type})
        if (t != HIPNLP_EXPR_SKIP && t != HIPNLP_EXPR_SUBJECT_TO && t != HIPNLP_EXPR_MINIMIZE) return fail(HIPNLP_E_INVALID, "bad expression type");
    if (desc->batch < 1) return fail(HIPNLP_E_INVALID, "batch must be >= 1");
    h->batch = desc->batch;
    std::string e;
    if (!Layout::make_kin_tables(desc->model, h->kt, e)) return fail(HIPNLP_E_INVALID, e);
    Layout::fill_terrain_tops(h->kt, st.terrain, st.n_terrain_steps, st.terrain_steps);
    if (!h->L.build(st, h->kt)) return fail(HIPNLP_E_INVALID, h->L.error);
    if (h->L.nnz > POSE_MAX_NNZ) return fail(HIPNLP_E_INVALID, "internal: pose pattern larger than POSE_MAX_NNZ");
    if (h->L.m > POSE_MAX_M) return fail(HIPNLP_E_INVALID, "internal: more rows than POSE_MAX_M");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(HIPNLP_E_NODEVICE, "no HIP device available (the engine has no CPU fallback)");
    if (desc->device < 0 || desc->device >= ndev) return fail(HIPNLP_E_INVALID, "bad device ordinal");
    h->dev = desc->device;
#define CREATE_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(HIPNLP_E_NODEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
    CREATE_TRY(hipSetDevice(h->dev));
    CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CREATE_TRY(hipEventCreate(&h->ev0));
    CREATE_TRY(hipEventCreate(&h->ev1));
    const size_t B = size_t(h->batch), m = size_t(h->L.m), nnz = size_t(h->L.nnz);
    CREATE_TRY(hipMalloc(&h->d_tb, sizeof(PoseTables)));
    CREATE_TRY(hipMalloc(&h->d_x, B * POSE_NX * sizeof(double)));
    CREATE_TRY(hipMalloc(&h->d_pk, B * PK_STRIDE * sizeof(double)));
    CREATE_TRY(hipMalloc(&h->d_xr, B * XR_STRIDE * sizeof(double)));
    CREATE_TRY(hipMalloc(&h->d_gp, B * sizeof(GParams)));
    CREATE_TRY(hipMalloc(&h->d_f, B * sizeof(double)));
    CREATE_TRY(hipMalloc(&h->d_grad, B * POSE_NX * sizeof(double)));
    CREATE_TRY(hipMalloc(&h->d_g, B * m * sizeof(double)));
    CREATE_TRY(hipMalloc(&h->d_jac, B * nnz * sizeof(double)));
    CREATE_TRY(hipMalloc(&h->d_cost, B * POSE_NCT * sizeof(double)));
    CREATE_TRY(hipMalloc(&h->d_flags, B * sizeof(int32_t)));
    CREATE_TRY(hipHostMalloc(&h->h_x, B * POSE_NX * sizeof(double)));
    CREATE_TRY(hipHostMalloc(&h->h_f, B * sizeof(double)));
    CREATE_TRY(hipHostMalloc(&h->h_grad, B * POSE_NX * sizeof(double)));
    CREATE_TRY(hipHostMalloc(&h->h_g, B * m * sizeof(double)));
    CREATE_TRY(hipHostMalloc(&h->h_jac, B * nnz * sizeof(double)));
    CREATE_TRY(hipHostMalloc(&h->h_cost, B * POSE_NCT * sizeof(double)));
    CREATE_TRY(hipHostMalloc(&h->h_flags, B * sizeof(int32_t)));
    {
        void* dv = nullptr;
        CREATE_TRY(hipHostGetDevicePointer(&dv, h->h_x, 0)); h->hd_x = static_cast<double*>(dv);
        CREATE_TRY(hipHostGetDevicePointer(&dv, h->h_f, 0)); h->hd_f = static_cast<double*>(dv);
        CREATE_TRY(hipHostGetDevicePointer(&dv, h->h_grad, 0)); h->hd_grad = static_cast<double*>(dv);
        CREATE_TRY(hipHostGetDevicePointer(&dv, h->h_g, 0)); h->hd_g = static_cast<double*>(dv);
        CREATE_TRY(hipHostGetDevicePointer(&dv, h->h_jac, 0)); h->hd_jac = static_cast<double*>(dv);
        CREATE_TRY(hipHostGetDevicePointer(&dv, h->h_cost, 0)); h->hd_cost = static_cast<double*>(dv);
        CREATE_TRY(hipHostGetDevicePointer(&dv, h->h_flags, 0)); h->hd_flags = static_cast<int32_t*>(dv);
    }
    PoseTables* tb = new PoseTables();
    std::memset(tb, 0, sizeof(PoseTables));
    tb->head.kt = h->kt;
    tb->head.ks = PoseLayout::make_ksettings(st);
    tb->hands = PoseLayout::make_hands(st);
    for (int s = 0; s < gs::COUNT; ++s) tb->g_row[s] = h->L.g_row[size_t(s)];
    for (int r = 0; r < POSE_MAX_M; ++r) tb->row_slot[r] = -1;
    for (int s = 0; s < gs::COUNT; ++s) if (h->L.g_row[size_t(s)] >= 0) tb->row_slot[h->L.g_row[size_t(s)]] = s;   // (PoseLayout::build: every row in exactly one slot)
    for (int e = 0; e < h->L.nnz; ++e) {   // (the device table holds indices of the compacted staging)
        const int slot = h->L.jperm[size_t(e)];
        if (!pjs::kept(slot)) { delete tb; return fail(HIPNLP_E_INVALID, "internal: a Jacobian slot of the pose pattern outside the staged pieces (pose_body.h pjs)"); }
        tb->jperm[e] = pjs::index(slot);
    }
    tb->nnz = h->L.nnz; tb->m = h->L.m;
    for (int e = 0; e < h->L.hnnz; ++e) tb->hperm[e] = h->L.hperm[size_t(e)];
    tb->hnnz = h->L.hnnz;
    hipError_t ce = hipnlp_internal_memcpy(h->d_tb, tb, sizeof(PoseTables), hipMemcpyHostToDevice);
    delete tb;
    if (ce != hipSuccess) return fail(HIPNLP_E_NODEVICE, std::string("hipMemcpy tables: ") + hipGetErrorString(ce));
    {
        CREATE_TRY(hipMalloc(&h->d_pt, sizeof(PoseProdTables)));
        PoseProdTables* pt = new PoseProdTables();
        h->L.fill_product_tables(*pt);
        ce = hipnlp_internal_memcpy(h->d_pt, pt, sizeof(PoseProdTables), hipMemcpyHostToDevice);
        delete pt;
        if (ce != hipSuccess) return fail(HIPNLP_E_NODEVICE, std::string("hipMemcpy product tables: ") + hipGetErrorString(ce));
    }
    h->kkt_fits = h->L.kkt_fits();
    if (!h->kkt_fits) { h->kkt_error = h->L.error; h->L.error.clear(); }   // (not an error of the handle: the three KKT entry points refuse)
    else {
        CREATE_TRY(hipMalloc(&h->d_kt, sizeof(PoseKktTables)));
        PoseKktTables* kt = new PoseKktTables();
        h->L.fill_kkt_tables(*kt);
        ce = hipnlp_internal_memcpy(h->d_kt, kt, sizeof(PoseKktTables), hipMemcpyHostToDevice);
        delete kt;
        if (ce != hipSuccess) return fail(HIPNLP_E_NODEVICE, std::string("hipMemcpy KKT tables: ") + hipGetErrorString(ce));
    }
    h->ldl_fits = h->L.ldl_fits();
    if (!h->ldl_fits) { h->ldl_error = h->L.error; h->L.error.clear(); }   // (not an error of the handle: the factorisation's entry points refuse)
    else {
        CREATE_TRY(hipMalloc(&h->d_lt, sizeof(PoseLdlTables)));
        PoseLdlTables* lt = new PoseLdlTables();
        h->L.fill_ldl_tables(*lt);
        ce = hipnlp_internal_memcpy(h->d_lt, lt, sizeof(PoseLdlTables), hipMemcpyHostToDevice);
        delete lt;
        if (ce != hipSuccess) return fail(HIPNLP_E_NODEVICE, std::string("hipMemcpy LDL table: ") + hipGetErrorString(ce));
    }
#undef CREATE_TRY
    *out = h;
    return HIPNLP_OK;
}

void hipnlp_pose_destroy(hipnlp_pose_handle* h) { pose_free_all(h); }

int hipnlp_pose_get_dims(const hipnlp_pose_handle* h, hipnlp_pose_dims* o) {
    if (!h || !o) return HIPNLP_E_INVALID;
    o->n = POSE_NX; o->m = h->L.m; o->nnz = h->L.nnz; o->np = POSE_NP;
    return HIPNLP_OK;
}

int hipnlp_pose_set_params(hipnlp_pose_handle* h, const double* p) {
    if (!h || !p) return HIPNLP_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->dev));
    const size_t B = size_t(h->batch);
    h->p.assign(p, p + B * POSE_NP);
    std::vector<double> pk(B * PK_STRIDE), xr(B * XR_STRIDE);
    std::vector<GParams> gp(B);
    for (size_t b = 0; b < B; ++b) pack_pose_params(p + b * POSE_NP, pk.data() + b * PK_STRIDE, xr.data() + b * XR_STRIDE, gp[b]);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipnlp_internal_memcpy(h->d_pk, pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipnlp_internal_memcpy(h->d_xr, xr.data(), xr.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipnlp_internal_memcpy(h->d_gp, gp.data(), gp.size() * sizeof(GParams), hipMemcpyHostToDevice));
    h->params_set = true;
    h->have_result = false;
    return HIPNLP_OK;
}

int hipnlp_pose_bounds(const hipnlp_pose_handle* h, double* lbg, double* ubg) {
    if (!h || !lbg || !ubg) return HIPNLP_E_INVALID;
    if (!h->params_set) return HIPNLP_E_PARAMS;
    for (int b = 0; b < h->batch; ++b) h->L.bounds(h->p.data() + size_t(b) * POSE_NP, lbg + size_t(b) * size_t(h->L.m), ubg + size_t(b) * size_t(h->L.m));
    return HIPNLP_OK;
}

int hipnlp_pose_sparsity(const hipnlp_pose_handle* h, int32_t* irow, int32_t* jcol) {
    if (!h || !irow || !jcol) return HIPNLP_E_INVALID;
    std::memcpy(irow, h->L.irow.data(), size_t(h->L.nnz) * sizeof(int32_t));
    std::memcpy(jcol, h->L.jcol.data(), size_t(h->L.nnz) * sizeof(int32_t));
    return HIPNLP_OK;
}

int hipnlp_pose_eval_device(hipnlp_pose_handle* h, const double* x_dev, double* f_dev, double* grad_dev, double* g_dev, double* jac_dev, void* stream) {
    if (!h || !x_dev) return HIPNLP_E_INVALID;
    if (!h->params_set) { h->err = "parameters not set (hipnlp_pose_set_params)"; return HIPNLP_E_PARAMS; }
    HIP_TRY(h, hipSetDevice(h->dev));
    h->have_result = false;
    return pose_launch(h, x_dev, f_dev ? f_dev : h->d_f, grad_dev, g_dev, jac_dev, stream ? hipStream_t(stream) : h->stream, false);
}

int hipnlp_pose_eval(hipnlp_pose_handle* h, const double* x, double* f, double* grad_f, double* g, double* jac) {
    if (!h || !x) return HIPNLP_E_INVALID;
    if (!h->params_set) { h->err = "parameters not set (hipnlp_pose_set_params)"; return HIPNLP_E_PARAMS; }
    const size_t B = size_t(h->batch), m = size_t(h->L.m), nnz = size_t(h->L.nnz);
    HIP_TRY(h, hipSetDevice(h->dev));
    // x is read by the kernel from the pinned staging copy, every output is stored by the kernel into its pinned block (PCIe stores):
    // one launch and one synchronisation, no copy command (56 -> 31 us per call for one pose through the ctypes binding, the Hessian 63 -> 42 us; tools/diag/pose_host_time.py)
    std::memcpy(h->h_x, x, B * POSE_NX * sizeof(double));
    const int rc = pose_launch(h, h->hd_x, h->hd_f, h->hd_grad, h->hd_g, h->hd_jac, h->stream, h->time_host, true);
    if (rc != HIPNLP_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->have_result = true;
    if (f) std::memcpy(f, h->h_f, B * sizeof(double));
    if (grad_f) std::memcpy(grad_f, h->h_grad, B * POSE_NX * sizeof(double));
    if (g) std::memcpy(g, h->h_g, B * m * sizeof(double));
    if (jac) std::memcpy(jac, h->h_jac, B * nnz * sizeof(double));
    for (size_t b = 0; b < B; ++b)
        if (h->h_flags[b]) { h->err = "non-finite value produced by the evaluation"; return HIPNLP_E_NUMERIC; }
    return HIPNLP_OK;
}

int hipnlp_pose_hess_nnz(const hipnlp_pose_handle* h, int32_t* nnz_h) {
    if (!h || !nnz_h) return HIPNLP_E_INVALID;
    *nnz_h = h->L.hnnz;
    return HIPNLP_OK;
}

int hipnlp_pose_hess_sparsity(const hipnlp_pose_handle* h, int32_t* irow, int32_t* jcol) {
    if (!h || !irow || !jcol) return HIPNLP_E_INVALID;
    std::memcpy(irow, h->L.hrow.data(), size_t(h->L.hnnz) * sizeof(int32_t));
    std::memcpy(jcol, h->L.hcol.data(), size_t(h->L.hnnz) * sizeof(int32_t));
    return HIPNLP_OK;
}

static int pose_hess_launch(hipnlp_pose_handle* h, const double* x_dev, const double* sigma_dev, const double* lambda_dev, double* hess_dev,
                            hipStream_t s, bool timed, bool host_block = false) {
    PArgs a{};
    a.tb = h->d_tb; a.x = x_dev; a.pk = h->d_pk; a.xr = h->d_xr; a.gp = h->d_gp;
    a.cost_terms = h->d_cost; a.flags = host_block ? h->hd_flags : h->d_flags;
    a.sigma = sigma_dev; a.lambda = lambda_dev; a.hess = hess_dev; a.m = h->L.m;
#ifdef HIPNLP_STAMPS
    if (!h->d_stamps) { HIP_TRY(h, hipMalloc(&h->d_stamps, size_t(h->batch) * 256 * sizeof(unsigned long long))); HIP_TRY(h, hipMemset(h->d_stamps, 0, size_t(h->batch) * 256 * sizeof(unsigned long long))); }
    a.stamps = h->d_stamps;
#endif
    if (timed) HIP_TRY(h, hipEventRecord(h->ev0, s));
    if (h->d.settings.terrain == HIPNLP_TERRAIN_PLANAR)
        hipLaunchKernelGGL(hipnlp_pose_hess_kernel<HIPNLP_TERRAIN_PLANAR>, dim3(unsigned(h->batch)), dim3(WG), 0, s, a);
    else
        hipLaunchKernelGGL(hipnlp_pose_hess_kernel<HIPNLP_TERRAIN_SMOOTH_STEPS>, dim3(unsigned(h->batch)), dim3(WG), 0, s, a);
    if (timed) HIP_TRY(h, hipEventRecord(h->ev1, s));
    HIP_TRY(h, hipGetLastError());
    if (timed) h->timing_valid = true;
    return HIPNLP_OK;
}

int hipnlp_pose_eval_hess_device(hipnlp_pose_handle* h, const double* x_dev, const double* obj_factor_dev, const double* lambda_dev,
                                 double* hess_dev, void* stream) {
    if (!h || !x_dev || !obj_factor_dev || !lambda_dev || !hess_dev) return HIPNLP_E_INVALID;
    if (!h->params_set) { h->err = "parameters not set (hipnlp_pose_set_params)"; return HIPNLP_E_PARAMS; }
    HIP_TRY(h, hipSetDevice(h->dev));
    return pose_hess_launch(h, x_dev, obj_factor_dev, lambda_dev, hess_dev, stream ? hipStream_t(stream) : h->stream, false);
}

int hipnlp_pose_eval_hess(hipnlp_pose_handle* h, const double* x, const double* obj_factor, const double* lambda, double* hess) {
    if (!h || !x || !obj_factor || !lambda || !hess) return HIPNLP_E_INVALID;
    if (!h->params_set) { h->err = "parameters not set (hipnlp_pose_set_params)"; return HIPNLP_E_PARAMS; }
    const size_t B = size_t(h->batch), m = size_t(h->L.m), hn = size_t(h->L.hnnz);
    HIP_TRY(h, hipSetDevice(h->dev));
    // every piece allocated at most once: a failure half way leaves the pieces that exist for the next attempt (nothing leaks)
    // pinned blocks, each with its device-visible address: the kernel gathers the multipliers out of host memory (m words per pose:
    // the rows of ONE pose) and stores the values into host memory; no copy command
    auto pinned = [&](double*& hostp, double*& devp, size_t count) -> int {
        if (!hostp) {
            HIP_TRY(h, hipHostMalloc(&hostp, count * sizeof(double)));
            void* dv = nullptr;
            HIP_TRY(h, hipHostGetDevicePointer(&dv, hostp, 0));
            devp = static_cast<double*>(dv);
        }
        return HIPNLP_OK;
    };
    int prc = pinned(h->h_sigma, h->hd_sigma, B);
    if (prc == HIPNLP_OK) prc = pinned(h->h_lambda, h->hd_lambda, B * m);
    if (prc == HIPNLP_OK) prc = pinned(h->h_hess, h->hd_hess, B * hn);
    if (prc != HIPNLP_OK) return prc;
    std::memcpy(h->h_x, x, B * POSE_NX * sizeof(double));
    std::memcpy(h->h_sigma, obj_factor, B * sizeof(double));
    std::memcpy(h->h_lambda, lambda, B * m * sizeof(double));
    const int rc = pose_hess_launch(h, h->hd_x, h->hd_sigma, h->hd_lambda, h->hd_hess, h->stream, h->time_host, true);
    if (rc != HIPNLP_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::memcpy(hess, h->h_hess, B * hn * sizeof(double));
    for (size_t b = 0; b < B; ++b)
        if (h->h_flags[b]) { h->err = "non-finite value produced by the evaluation"; return HIPNLP_E_NUMERIC; }
    return HIPNLP_OK;
}

// ---- workgroup-local products (pose_products.h): one launch each, device pointers, no host copy --------------------------------------
enum { POSE_PROD_LGRAD, POSE_PROD_JVP, POSE_PROD_HVP };
static int pose_product_launch(hipnlp_pose_handle* h, int which, const double* x_dev, const double* sigma_dev, const double* lambda_dev, const double* v_dev,
                               double* out_dev, double* dot_dev, void* stream) {
    if (!h->params_set) { h->err = "parameters not set (hipnlp_pose_set_params)"; return HIPNLP_E_PARAMS; }
    HIP_TRY(h, hipSetDevice(h->dev));
    h->have_result = false;
    PPArgs pa{};
    PArgs& a = pa.p;
    a.tb = h->d_tb; a.x = x_dev; a.pk = h->d_pk; a.xr = h->d_xr; a.gp = h->d_gp;
    a.cost_terms = h->d_cost; a.flags = h->d_flags;
    a.sigma = sigma_dev; a.lambda = lambda_dev; a.m = h->L.m;
    pa.pt = h->d_pt; pa.v = v_dev; pa.out = out_dev; pa.dot = dot_dev;
    hipStream_t s = stream ? hipStream_t(stream) : h->stream;
    const dim3 grid(unsigned(h->batch)), block(WG);
    const bool planar = h->d.settings.terrain == HIPNLP_TERRAIN_PLANAR;
    switch (which) {
        case POSE_PROD_LGRAD:
            if (planar) hipLaunchKernelGGL(hipnlp_pose_lgrad_kernel<HIPNLP_TERRAIN_PLANAR>, grid, block, 0, s, pa);
            else hipLaunchKernelGGL(hipnlp_pose_lgrad_kernel<HIPNLP_TERRAIN_SMOOTH_STEPS>, grid, block, 0, s, pa);
            break;
        case POSE_PROD_JVP:
            if (planar) hipLaunchKernelGGL(hipnlp_pose_jvp_kernel<HIPNLP_TERRAIN_PLANAR>, grid, block, 0, s, pa);
            else hipLaunchKernelGGL(hipnlp_pose_jvp_kernel<HIPNLP_TERRAIN_SMOOTH_STEPS>, grid, block, 0, s, pa);
            break;
        default:
            if (planar) hipLaunchKernelGGL(hipnlp_pose_hvp_kernel<HIPNLP_TERRAIN_PLANAR>, grid, block, 0, s, pa);
            else hipLaunchKernelGGL(hipnlp_pose_hvp_kernel<HIPNLP_TERRAIN_SMOOTH_STEPS>, grid, block, 0, s, pa);
            break;
    }
    HIP_TRY(h, hipGetLastError());
    return HIPNLP_OK;
}

int hipnlp_pose_eval_lagrangian_grad_device(hipnlp_pose_handle* h, const double* x_dev, const double* obj_factor_dev, const double* lambda_dev,
                                            double* out_dev, void* stream) {
    if (!h || !x_dev || !obj_factor_dev || !lambda_dev || !out_dev) return HIPNLP_E_INVALID;
    return pose_product_launch(h, POSE_PROD_LGRAD, x_dev, obj_factor_dev, lambda_dev, nullptr, out_dev, nullptr, stream);
}

int hipnlp_pose_eval_jac_vec_device(hipnlp_pose_handle* h, const double* x_dev, const double* v_dev, double* gradf_dot_v_dev, double* jac_v_dev, void* stream) {
    if (!h || !x_dev || !v_dev || (!gradf_dot_v_dev && !jac_v_dev)) return HIPNLP_E_INVALID;
    return pose_product_launch(h, POSE_PROD_JVP, x_dev, nullptr, nullptr, v_dev, jac_v_dev, gradf_dot_v_dev, stream);
}

int hipnlp_pose_eval_hess_vec_device(hipnlp_pose_handle* h, const double* x_dev, const double* obj_factor_dev, const double* lambda_dev,
                                     const double* v_dev, double* out_dev, void* stream) {
    if (!h || !x_dev || !obj_factor_dev || !lambda_dev || !v_dev || !out_dev) return HIPNLP_E_INVALID;
    return pose_product_launch(h, POSE_PROD_HVP, x_dev, obj_factor_dev, lambda_dev, v_dev, out_dev, nullptr, stream);
}

// ---- the KKT chain from stored value runs (pose_kkt.h): one launch each, device pointers, no host copy, no workspace ----------------------
enum { POSE_KKT_TIMES, POSE_KKT_DIAG, POSE_KKT_SOLVE };
static int pose_kkt_launch(hipnlp_pose_handle* h, const char* who, int which, PKArgs& a, void* stream) {
    if (!h->kkt_fits) { h->err = std::string(who) + ": " + h->kkt_error; return HIPNLP_E_UNSUPPORTED; }
    HIP_TRY(h, hipSetDevice(h->dev));
    a.kt = h->d_kt; a.pt = h->d_pt;
    a.m = h->L.m; a.nnz = h->L.nnz; a.hnnz = h->L.hnnz;
    hipStream_t s = stream ? hipStream_t(stream) : h->stream;
    const dim3 grid(unsigned(h->batch)), block(WG);
    switch (which) {
        case POSE_KKT_TIMES: hipLaunchKernelGGL(hipnlp_pose_saddle_times_kernel, grid, block, 0, s, a); break;
        case POSE_KKT_DIAG: hipLaunchKernelGGL(hipnlp_pose_saddle_diag_kernel, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(hipnlp_pose_saddle_solve_kernel, grid, block, 0, s, a); break;
    }
    HIP_TRY(h, hipGetLastError());
    return HIPNLP_OK;
}

int hipnlp_pose_kkt_times_device(hipnlp_pose_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* v_dev, const double* w_dev,
                                 double* top_dev, double* bottom_dev, const double* dx_dev, const double* dc_dev, void* stream) {
    if (!h) return HIPNLP_E_INVALID;
    if (!hess_values_dev || !jac_values_dev || !v_dev || !w_dev || !top_dev || !bottom_dev) { h->err = "hipnlp_pose_kkt_times_device: a required pointer is null"; return HIPNLP_E_INVALID; }
    PKArgs a{};
    a.hess = hess_values_dev; a.jac = jac_values_dev; a.in_top = v_dev; a.in_bot = w_dev; a.out_top = top_dev; a.out_bot = bottom_dev; a.dx = dx_dev; a.dc = dc_dev;
    return pose_kkt_launch(h, "hipnlp_pose_kkt_times_device", POSE_KKT_TIMES, a, stream);
}

int hipnlp_pose_kkt_diag_precond_device(hipnlp_pose_handle* h, const double* hess_values_dev, const double* jac_values_dev, double* minv_top_dev, double* minv_bottom_dev,
                                        const double* dx_dev, const double* dc_dev, double floor, void* stream) {
    if (!h) return HIPNLP_E_INVALID;
    if (!hess_values_dev || !jac_values_dev || !minv_top_dev || !minv_bottom_dev) { h->err = "hipnlp_pose_kkt_diag_precond_device: a required pointer is null"; return HIPNLP_E_INVALID; }
    if (!(floor > 0.0) || !minres_finite(floor)) { h->err = "hipnlp_pose_kkt_diag_precond_device: floor must be a finite number > 0"; return HIPNLP_E_INVALID; }
    PKArgs a{};
    a.hess = hess_values_dev; a.jac = jac_values_dev; a.out_top = minv_top_dev; a.out_bot = minv_bottom_dev; a.dx = dx_dev; a.dc = dc_dev; a.floor = floor;
    return pose_kkt_launch(h, "hipnlp_pose_kkt_diag_precond_device", POSE_KKT_DIAG, a, stream);
}

int hipnlp_pose_kkt_minres_device(hipnlp_pose_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* rhs_top_dev, const double* rhs_bottom_dev,
                                  double* sol_top_dev, double* sol_bottom_dev, int32_t* iterations_dev, double* residual_dev, int32_t* status_dev, const double* dx_dev,
                                  const double* dc_dev, const double* minv_top_dev, const double* minv_bottom_dev, int build_diagonal, double floor, double rtol,
                                  int max_iterations, void* stream) {
    if (!h) return HIPNLP_E_INVALID;
    if (!hess_values_dev || !jac_values_dev || !rhs_top_dev || !rhs_bottom_dev || !sol_top_dev || !sol_bottom_dev || !iterations_dev || !residual_dev || !status_dev) {
        h->err = "hipnlp_pose_kkt_minres_device: a required pointer is null";
        return HIPNLP_E_INVALID;
    }
    if (!(rtol >= 0.0) || max_iterations < 0 || max_iterations > PK_MAX_ITERATIONS || (minv_top_dev == nullptr) != (minv_bottom_dev == nullptr) ||
        (build_diagonal && minv_top_dev) || !(floor > 0.0) || !minres_finite(floor)) {
        h->err = "hipnlp_pose_kkt_minres_device: rtol >= 0, 0 <= max_iterations <= " + std::to_string(PK_MAX_ITERATIONS) +
                 " (one launch runs them all), both or neither of minv_top_dev / minv_bottom_dev and neither with build_diagonal, a finite floor > 0";
        return HIPNLP_E_INVALID;
    }
    PKArgs a{};
    a.hess = hess_values_dev; a.jac = jac_values_dev; a.in_top = rhs_top_dev; a.in_bot = rhs_bottom_dev; a.out_top = sol_top_dev; a.out_bot = sol_bottom_dev;
    a.iterations = iterations_dev; a.residual = residual_dev; a.status = status_dev; a.dx = dx_dev; a.dc = dc_dev; a.minv_top = minv_top_dev; a.minv_bot = minv_bottom_dev;
    a.build_diag = build_diagonal != 0; a.floor = floor; a.rtol = rtol; a.maxit = max_iterations;
    return pose_kkt_launch(h, "hipnlp_pose_kkt_minres_device", POSE_KKT_SOLVE, a, stream);
}

// ---- the dense L D L^T of the KKT matrix per pose (pose_ldl.h): one launch each, device pointers, no workspace ------------------------------
int hipnlp_pose_kkt_ldl_doubles(const hipnlp_pose_handle* h) {
    if (!h) return HIPNLP_E_INVALID;
    if (!h->ldl_fits) return HIPNLP_E_UNSUPPORTED;
    return pl_doubles(POSE_NX + h->L.m);
}

static int pose_ldl_launch(hipnlp_pose_handle* h, const char* who, bool factor, PLArgs& a, void* stream) {
    if (!h->ldl_fits) { h->err = std::string(who) + ": " + h->ldl_error; return HIPNLP_E_UNSUPPORTED; }
    HIP_TRY(h, hipSetDevice(h->dev));
    a.lt = h->d_lt;
    a.m = h->L.m; a.nnz = h->L.nnz; a.hnnz = h->L.hnnz;
    hipStream_t s = stream ? hipStream_t(stream) : h->stream;
    const dim3 grid(unsigned(h->batch)), block(LDL_WG);
    if (factor) hipLaunchKernelGGL(hipnlp_pose_saddle_ldl_kernel, grid, block, 0, s, a);
    else hipLaunchKernelGGL(hipnlp_pose_saddle_ldl_solve_kernel, grid, block, 0, s, a);
    HIP_TRY(h, hipGetLastError());
    return HIPNLP_OK;
}

int hipnlp_pose_kkt_ldl_device(hipnlp_pose_handle* h, const double* hess_values_dev, const double* jac_values_dev, const double* dx_dev, const double* dc_dev, int nrhs,
                               const double* rhs_top_dev, const double* rhs_bottom_dev, double* sol_top_dev, double* sol_bottom_dev, int32_t* inertia_dev, int32_t* status_dev,
                               double* delta_dev, int32_t* tries_dev, double delta_init, double kappa, int max_tries, double* factor_dev, int32_t* pivots_dev, void* stream) {
    if (!h) return HIPNLP_E_INVALID;
    if (const char* e = pl_factor_call_error(hess_values_dev, jac_values_dev, nrhs, rhs_top_dev, rhs_bottom_dev, sol_top_dev, sol_bottom_dev, inertia_dev, status_dev, delta_init,
                                             kappa, max_tries, factor_dev, pivots_dev)) {
        h->err = std::string("hipnlp_pose_kkt_ldl_device: ") + e;
        return HIPNLP_E_INVALID;
    }
    PLArgs a{};
    a.hess = hess_values_dev; a.jac = jac_values_dev; a.dx = dx_dev; a.dc = dc_dev; a.nrhs = nrhs;
    a.rhs_top = rhs_top_dev; a.rhs_bot = rhs_bottom_dev; a.sol_top = sol_top_dev; a.sol_bot = sol_bottom_dev;
    a.inertia = inertia_dev; a.status = status_dev; a.delta = delta_dev; a.tries = tries_dev;
    a.delta_init = max_tries > 0 ? delta_init : 0.0; a.kappa = max_tries > 0 ? kappa : 0.0; a.max_tries = max_tries;
    a.factor = factor_dev; a.pivots = pivots_dev;
    return pose_ldl_launch(h, "hipnlp_pose_kkt_ldl_device", true, a, stream);
}

int hipnlp_pose_kkt_ldl_solve_device(hipnlp_pose_handle* h, const double* factor_dev, const int32_t* pivots_dev, int nrhs, const double* rhs_top_dev,
                                     const double* rhs_bottom_dev, double* sol_top_dev, double* sol_bottom_dev, void* stream) {
    if (!h) return HIPNLP_E_INVALID;
    if (const char* e = pl_solve_call_error(factor_dev, pivots_dev, nrhs, rhs_top_dev, rhs_bottom_dev, sol_top_dev, sol_bottom_dev)) {
        h->err = std::string("hipnlp_pose_kkt_ldl_solve_device: ") + e;
        return HIPNLP_E_INVALID;
    }
    PLArgs a{};
    a.factor = const_cast<double*>(factor_dev); a.pivots = const_cast<int32_t*>(pivots_dev); a.nrhs = nrhs;       // (sources here: the solve kernel stores to neither)
    a.rhs_top = rhs_top_dev; a.rhs_bot = rhs_bottom_dev; a.sol_top = sol_top_dev; a.sol_bot = sol_bottom_dev;
    return pose_ldl_launch(h, "hipnlp_pose_kkt_ldl_solve_device", false, a, stream);
}

int hipnlp_pose_cost_terms(hipnlp_pose_handle* h, double* values) {
    if (!h || !values) return HIPNLP_E_INVALID;
    if (!h->have_result) {
        HIP_TRY(h, hipSetDevice(h->dev));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipnlp_internal_memcpy(h->h_cost, h->d_cost, size_t(h->batch) * POSE_NCT * sizeof(double), hipMemcpyDeviceToHost));
    }
    std::memcpy(values, h->h_cost, size_t(h->batch) * POSE_NCT * sizeof(double));
    return HIPNLP_OK;
}

const char* hipnlp_pose_cost_term_name(int i) {
    static const char* names[POSE_NCT] = {"base_quaternion_error", "frame_rotation_error", "com_position_error", "joint_positions_error",
                                          "average_force_regularization", "point_position_regularization", "force_regularization",
                                          "left_hand_position_error", "right_hand_position_error"};
    return (i >= 0 && i < POSE_NCT) ? names[i] : "";
}

int hipnlp_pose_num_row_blocks(const hipnlp_pose_handle* h) { return h ? int(h->L.blocks.size()) : HIPNLP_E_INVALID; }

int hipnlp_pose_row_block(const hipnlp_pose_handle* h, int i, const char** name, int32_t* first_row, int32_t* rows) {
    if (!h || i < 0 || i >= int(h->L.blocks.size())) return HIPNLP_E_INVALID;
    const PoseRowBlock& b = h->L.blocks[size_t(i)];
    if (name) *name = b.name.c_str();
    if (first_row) *first_row = b.first_row;
    if (rows) *rows = b.rows;
    return HIPNLP_OK;
}

int hipnlp_pose_set_host_timing(hipnlp_pose_handle* h, int on) {
    if (!h) return HIPNLP_E_INVALID;
    h->time_host = on != 0;
    if (!h->time_host) h->timing_valid = false;
    return HIPNLP_OK;
}

int hipnlp_pose_last_kernel_ms(hipnlp_pose_handle* h, float* ms) {
    if (!h || !ms) return HIPNLP_E_INVALID;
    if (!h->timing_valid) { h->err = "no timed evaluation yet (hipnlp_pose_set_host_timing(h, 1), then hipnlp_pose_eval / hipnlp_pose_eval_hess)"; return HIPNLP_E_INVALID; }
    HIP_TRY(h, hipSetDevice(h->dev));
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    HIP_TRY(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return HIPNLP_OK;
}

#ifdef HIPNLP_STAMPS
int hipnlp_pose_debug_stamps(hipnlp_pose_handle* h, unsigned long long* out /*[batch][4][64]*/) {
    if (!h || !out || !h->d_stamps) return HIPNLP_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->dev));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipnlp_internal_memcpy(out, h->d_stamps, size_t(h->batch) * 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return HIPNLP_OK;
}
#endif

}  // extern "C"
