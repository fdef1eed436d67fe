// TEST-ONLY CPU emulation of the per-knot inertia-correcting ladder of the block factorisation (hipnlp.hip hipnlp_kkt_block_ladder_kernel):
// the ladder's text — the delta of a try, whether another try follows, the inertia that is wanted, the final status — is knot_ldl.h's
// and pose_ldl.h's, the headers the device compiles; the assembly of a try is written here from the vectors of HessLayout and walked from
// the last element down, and the factorisation is tests/kkt_block_emu's, in its own element order.  One factorisation at an EXPLICIT delta
// is exposed beside the ladder, so that a test can climb the ladder by hand.  The block preconditioner's, the diagonal's, the solve's and
// the operator's emulations are compiled into this library as they stand, so that all of them share one handle.  It is NOT part of the
// product: libhipnlp.so does not contain it.
#include "../kkt_block_emu/kkt_block_emu.cpp"

namespace {

// one try of one knot: assembly with (H_cc + dx_c) + delta where with_delta, else tests/kkt_block_emu's block_record; the whole record
BlockFactored ladder_try(const HessLayout& HL, const double* hess, const double* dx, double floor, bool with_delta, double delta, double* factor, int* words, double* e, double* o,
                         int* not_pd) {
    constexpr int N = KL_N;
    std::vector<int> ipiv(size_t(N), 0), perm(size_t(N), 0), kind(size_t(N), 0);
    for (int q = KL_DOUBLES - 1; q >= 0; --q) factor[q] = 0.0;
    for (int p = HL.nnz_knot - 1; p >= 0; --p) factor[pl_at(N, HL.lrow[size_t(p)], HL.lcol[size_t(p)])] = hess[p];
    for (int c = N - 1; c >= 0; --c) factor[pl_col(N, c)] = pl_diag_top(factor[pl_col(N, c)], dx != nullptr, dx ? dx[c] : 0.0, with_delta, delta);
    BlockFactored f = block_factor(factor, ipiv.data(), perm.data(), kind.data());
    if (f.status != KL_OK) {
        for (int q = 0; q < KL_DOUBLES; ++q) factor[q] = pl_nan();
        for (int i = 0; i < N; ++i) { words[i] = kl_word(i + 1, i, PL_ONE); e[i] = o[i] = pl_nan(); }
        f.pos = f.neg = f.zero = 0;
        return f;
    }
    for (int i = N - 1; i >= 0; --i) {
        words[i] = kl_word(ipiv[size_t(i)], perm[size_t(i)], kind[size_t(i)]);
        o[i] = 0.0;
        if (kind[size_t(i)] == PL_ONE) e[i] = kl_floored_inverse(factor[pl_col(N, i)], floor);
        else if (kind[size_t(i)] == PL_FIRST) {
            const KlAbsInv2 q = kl_abs_inverse2(factor[pl_col(N, i)], factor[pl_col(N, i) + 1], factor[pl_col(N, i + 1)], floor);
            e[i] = q.e0; o[i] = q.o;
            if (!kl_block_positive_definite(q.e0, q.e1, q.o)) ++*not_pd;
        } else e[i] = kl_abs_inverse2(factor[pl_col(N, i - 1)], factor[pl_col(N, i - 1) + 1], factor[pl_col(N, i)], floor).e1;
    }
    return f;
}

}  // namespace

extern "C" {

// [0] PL_MAX_TRIES, [1] KL_OK, [2] KL_NONFINITE, [3] KL_EXHAUSTED
void klemu_caps(int* out) { out[0] = PL_MAX_TRIES; out[1] = KL_OK; out[2] = KL_NONFINITE; out[3] = KL_EXHAUSTED; }

// ONE factorisation of knot k at an explicit delta (with_delta = 0: try 0's assembly, delta not read): factor [KL_DOUBLES], words / e / o
// [189], inertia [3], status [1] — the raw status of the try (KL_OK or KL_NONFINITE), the inertia (0, 0, 0) with KL_NONFINITE
void klemu_factor_at(const kktemu_handle* h, int k, const double* hess, const double* dx, double floor, int with_delta, double delta, double* factor, int* words, double* e,
                     double* o, int* inertia, int* status) {
    int not_pd = 0;
    const BlockFactored f = ladder_try(h->HL, hess + h->HL.knot_base(k), dx ? dx + size_t(NXK) * k : nullptr, floor, with_delta != 0, delta, factor, words, e, o, &not_pd);
    inertia[0] = f.pos; inertia[1] = f.neg; inertia[2] = f.zero;
    status[0] = f.status;
}

// hipnlp_kkt_block_ladder_kernel, one trajectory: kbemu_factor's arrays plus delta [N] and tries [N]
void klemu_ladder(const kktemu_handle* h, const double* hess, const double* dx, double floor, double delta_init, double kappa, int max_tries, double* factor, int* words, double* e,
                  double* o, int* inertia, int* status, double* delta_out, int* tries_out, int* checks) {
    const int N = h->L.N;
    checks[0] = checks[1] = 0;
    for (int k = N - 1; k >= 0; --k) {   // (the knots are independent: any order)
        double delta = 0.0;
        int t = 0;
        BlockFactored f;
        bool wanted = false;
        for (;;) {
            int not_pd = 0;
            f = ladder_try(h->HL, hess + h->HL.knot_base(k), dx ? dx + size_t(NXK) * k : nullptr, floor, t > 0, delta, factor + size_t(k) * KL_DOUBLES, words + size_t(k) * KL_N,
                           e + size_t(k) * KL_N, o + size_t(k) * KL_N, &not_pd);
            wanted = kl_inertia_wanted(f.pos, f.neg, f.zero);
            if (!pl_ladder_goes_on(f.status, wanted, t, max_tries)) { checks[0] += f.det_not_negative; checks[1] += not_pd; break; }
            ++t;
            delta = pl_next_delta(t, delta, delta_init, kappa);
        }
        inertia[3 * k + 0] = f.pos; inertia[3 * k + 1] = f.neg; inertia[3 * k + 2] = f.zero;
        status[k] = kl_ladder_final_status(f.status, wanted, max_tries);
        delta_out[k] = delta;
        tries_out[k] = t;
    }
}

// what the entry point refuses (knot_ldl.h): 1 and the reason in msg, or 0
int klemu_ladder_call_error(int hess, double floor, double delta_init, double kappa, int max_tries, int factor, int pivots, int e, int o, int inertia, int status, int delta, int tries,
                            char* msg, int msglen) {
    const char* r = kl_ladder_call_error(hess, floor, delta_init, kappa, max_tries, factor, pivots, e, o, inertia, status, delta, tries);
    if (r) std::strncpy(msg, r, size_t(msglen - 1));
    return r != nullptr;
}

}  // extern "C"
