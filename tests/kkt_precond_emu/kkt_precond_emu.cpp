// TEST-ONLY CPU emulation of hipnlp_kkt_diag_precond_device (hipnlp.hip hipnlp_saddle_diag_kernel): the one launch walked workgroup by
// workgroup over the knots of ONE trajectory — per knot the four records of minv_top the workgroup computes for itself (own knot,
// predecessor, other horizon end, globals) from one gathered Hessian value and one d_x each, the phase-1 staging of the jac values as the
// operator's emulation does it (tests/kkt_emu), the owned rows over the JprodTables words, and the stores by minres_owned — with every
// expression of knot_kkt_precond.h, the same header the device compiles.  The operator's and the solve's emulations are compiled into this
// library as they stand, so that building the diagonal and solving with it share one handle.  It is NOT part of the product:
// libhipnlp.so does not contain it.
#include "../kkt_minres_emu/kkt_minres_emu.cpp"

#include "../../hippopt_amd/csrc/knot_kkt_precond.h"

extern "C" {

// the block position of the diagonal entry of every variable of a knot record (-1: none): HessLayout::hv_diag
void kpcemu_diag_positions(const kktemu_handle* h, int* pos) {
    for (int i = 0; i < NXK; ++i) pos[i] = h->HL.hv_diag[size_t(i)];
}

// minv_top [n], minv_bottom [m] from the value runs hess [nnz_h] and jac [nnz]; dx / dc may be null; top_writes [n] / bottom_writes [m]
// count the stores
void kpcemu_build(const kktemu_handle* h, const double* hess, const double* jac, const double* dx, const double* dc, double floor, double* minv_top, double* minv_bottom,
                  int* top_writes, int* bottom_writes) {
    const Layout& L = h->L;
    const HessLayout& HL = h->HL;
    const JprodTables& T = h->T;
    const int N = L.N;
    std::vector<double> js(JP_VALUES), ms(JP_V_WORDS);
    // minv_top of variable c of knot kk, as every workgroup that needs it computes it
    auto top_of = [&](int kk, int c) {
        const int p = HL.hv_diag[size_t(c)];
        const long i = long(NXK) * kk + c;
        return precond_top(dx != nullptr, p >= 0 ? hess[HL.knot_base(kk) + p] : 0.0, dx ? dx[i] : 0.0, floor);
    };
    auto glob_of = [&](int c) { return precond_top(dx != nullptr, 0.0, dx ? dx[long(NXK) * N + c] : 0.0, floor); };
    for (int k = 0; k < N; ++k) {
        const int pv = L.pair_variant_of(k);
        // the records of minv_top in the JP_V_* arrangement (zeros where a guard keeps the workgroup from computing one), and the jac values
        // as the operator's emulation stages them (tests/values_stage_emu.h)
        values_stage_emu::stage_records(k, N, ms.data(), top_of, glob_of);
        values_stage_emu::stage_jac_rows(L, T, jac, k, js.data());
        // the stores, thread by thread: what minres_owned gives the thread
        for (int tid = 0; tid < JP_WG; ++tid) {
            const MinresOwned o = minres_owned(tid, k, N, T.row_a[pv], T.row_b[pv]);
            if (o.top >= 0) {
                minv_top[o.top] = tid < NXK ? ms[size_t(tid)] : ms[size_t(JP_V_GLOB + (tid - JP_V_STRIDE))];
                top_writes[o.top]++;
            }
            for (int q = 0; q < 2; ++q) {
                if (o.row[q] < 0) continue;
                const long r = o.row[q];
                const double sum = precond_row_staged(T.rdir[pv][tid + q * JP_WG], T.word[pv], js.data(), ms.data());
                minv_bottom[r] = precond_bottom(dc != nullptr, dc ? dc[r] : 0.0, sum, floor);
                bottom_writes[r]++;
            }
        }
    }
}

}  // extern "C"
