"""The condensed block factorisation of the KKT solve (hippopt_amd/csrc/knot_condense.h), run by the CPU emulation of
hipnlp_kkt_condensed_factor_kernel (tests/kkt_condensed_emu) on the systems of tests/test_kkt_block_hostemu.py::real_runs (seed 8900, sigma
0.8, RandomState(11), the stairs on the flanks), at dx, dc in U[1, 2] and with both multiplied by 1e-4:

    B_k = H_k + diag dx_k + J_k^T diag(1 / dc) J_k,      C = H + diag dx + J^T diag(1 / dc) J,      In(K) = (0, m, 0) + In(C)

  1. the assembled B_k against dense numpy, element by element within gamma(T + 2) sum |terms|, T the element's number of fused
     multiply-adds; the pattern-driven emulation against the DEVICE tables and the device's merge, bit for bit; both jac orders the same
     bits; a jac run of zeros gives block_factor's six arrays;
  2. P B P^T = L D L^T within check_factorisation's bound, the inertia of every knot against eigvalsh's sign counts;
  3. dense N = 2: eigvalsh(K) has m + neg(C) negative values and neg(C) >= max_k neg(B_k) — what the docstrings say the inertia proves;
  4. MINRES with it, rtol 1e-8: at most half block_preconditioner's iterations at U[1, 2]; status 0 at 1e-4 where block_preconditioner
     stands at status 1 after 3 000; status 0 implies a true residual within 100 rtol in the M^-1 norm (the norm MINRES stops in);
  5. a NaN in one knot's Hessian, a dc_i that is <= 0, NaN or infinite, every output word written, N = 2.

SEEN with this emulation (iterations, rtol 1e-8, at most 3 000):
                          block_preconditioner    condensed    condensed diagonal alone
  periodic N=4  U[1,2]           315                  58              538
  stairs   N=4  U[1,2]           456                 133              988
  periodic N=2  x1e-4      status 1 (3 000)          155              309
  periodic N=4  x1e-4      status 1 (3 000)          247              489
  stairs   N=4  x1e-4      status 1 (3 000)          340            1 331
(block_preconditioner: the block factor with the Schur diagonal beside it, as KKTValues.block_preconditioner builds it; its residuals at
3 000: 1.1e-2, 3.0e-2, 1.8e-2.)  The true residual in the 2-norm is NOT within 100 rtol at 1e-4 (5.9e-5 periodic, 5.6e-4 stairs at N = 4):
M^-1 weighs the bottom rows by 1 / dc of about 1e4; MINRES minimises, and the tests assert, the M^-1 norm.  The reference of check 1 is
numpy in np.longdouble: in float64 the reference's own rounding is as large as the bound.
Inertia of B_k (negative eigenvalues per knot): periodic N=4 U[1,2] [4, 2, 0, 0], x1e-4 [0, 0, 0, 0]; stairs N=4 U[1,2] [12, 12, 13, 9], x1e-4
[2, 0, 0, 0].  Of the 36 blocks of both terrains at N = 2, 3, 4 and both scales none is undecidable for the reference (smallest |eigenvalue|
below 189 2^-53 max |eigenvalue|); the cap is one in ten.  Largest block: 1 620 entries (stairs, interior knot), 439 rows (periodic, last
knot), 14 144 pair terms.  CPU only."""
import numpy as np
import pytest

import kkt_check
from hvp_check import gamma
from kkt_check import bits
from kkt_emu_lib import NXK
from test_kkt_block_hostemu import dense_block, real_runs, split
from test_kkt_minres_hostemu import inputs
from test_lagrangian_grad_hostemu import MAKERS

U = 2.0 ** -53
FLOOR, RTOL = 1e-10, 1e-8
REAL = ["periodic", "stairs"]
SCALES = [1.0, 1e-4]
RECORD = ("factor", "words", "e", "o", "inertia", "status")
_EMU, _PAT, _FAC = {}, {}, {}


def emu_of(model, name, horizon, lifted=False, vary_first=False):
    from kkt_condensed_emu_lib import KktCondensedEmu
    key = (name, horizon, lifted, vary_first)
    if key not in _EMU:
        emu = KktCondensedEmu(MAKERS[name](horizon, model), model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
        _EMU[key] = emu
        _PAT[key] = tuple(np.asarray(a) for a in emu.hess_sparsity() + emu.sparsity())
    return _EMU[key], _PAT[key]


def runs(model, name, horizon, scale=1.0):
    """(this emulation, patterns, inputs) of real_runs with dx and dc multiplied by scale; real_runs' own arrays stay as they are"""
    _, pat, d = real_runs(model, name, horizon)
    emu, _ = emu_of(model, name, horizon)
    return emu, pat, (d if scale == 1.0 else dict(d, dx=d["dx"] * scale, dc=d["dc"] * scale))


def factored(model, name, horizon, scale=1.0):
    key = (name, horizon, scale)
    if key not in _FAC:
        emu, pat, d = runs(model, name, horizon, scale)
        _FAC[key] = emu.condensed_factor(d["hess"], d["jac"], d["dc"], d["dx"], FLOOR)
    return _FAC[key]


def unpack(a):
    """the packed lower triangle (column major) as a full symmetric matrix"""
    A, idx = np.zeros((NXK, NXK)), 0
    for j in range(NXK):
        A[j:, j] = a[idx:idx + NXK - j]
        idx += NXK - j
    return A + np.tril(A, -1).T


def column_block(emu, pat, jac, k):
    """(J_k [m, 189] dense, its pattern as 0 / 1) — the entries of jac g in the columns of knot k"""
    ir, jc = pat[2], pat[3]
    on = (jc >= NXK * k) & (jc < NXK * (k + 1))
    J, P = np.zeros((emu.m, NXK)), np.zeros((emu.m, NXK))
    J[ir[on], jc[on] - NXK * k] = jac[on]
    P[ir[on], jc[on] - NXK * k] = 1.0
    return J, P


def dense_condensed(emu, pat, d, k, exact=False):
    """(B_k, sum |terms| of every element, the number of pair terms of every element) in numpy: float64, or with exact=True in the
    extended precision of np.longdouble (a 64-bit significand here), whose own error is 2^-11 of the bound's unit"""
    J, P = column_block(emu, pat, d["jac"], k)
    H = dense_block(pat, d["hess"], None, k)
    dxk = d["dx"][NXK * k:NXK * (k + 1)] if d["dx"] is not None else np.zeros(NXK)
    rows = np.flatnonzero(P.any(axis=1))                                             # the rows touching the block
    if exact:
        H, dxk, J = H.astype(np.longdouble), dxk.astype(np.longdouble), J.astype(np.longdouble)
        s = 1.0 / d["dc"][rows].astype(np.longdouble)
    else:
        s = 1.0 / d["dc"][rows]
    Jr = J[rows]
    B = H + np.diag(dxk) + Jr.T @ (s[:, None] * Jr)
    mag = np.abs(H) + np.diag(np.abs(dxk)) + np.abs(Jr).T @ (s[:, None] * np.abs(Jr))
    return B, mag, np.rint(P.T @ P).astype(np.int64)


def check_block(emu, pat, d, k, what):
    a, terms, good = emu.condensed_block(k, d["hess"], d["jac"], d["dc"], d["dx"])
    B, mag, T = dense_condensed(emu, pat, d, k, exact=True)
    assert good and np.finfo(np.longdouble).nmant >= 63                              # the reference is more precise than what it checks
    got, tt = unpack(a), unpack(terms.astype(np.float64)).astype(np.int64)
    assert np.array_equal(tt, T), (what, k)                                          # one fused multiply-add per common row, no more
    bound = np.vectorize(gamma)(T + 2) * mag
    err = np.abs(got.astype(np.longdouble) - B).astype(np.float64)
    bound = bound.astype(np.float64)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print("%s knot %d: %d pair terms, at most %d per element; |B - numpy| at most %.3f of gamma(T + 2) sum |terms|" % (what, k, np.tril(T).sum(), T.max(), worst))
    assert np.all(err <= bound), (what, k, worst)
    return a


# ---- 1. the assembled block -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("horizon", [2, 3, 4])
@pytest.mark.parametrize("name", REAL)
def test_the_assembled_block_against_numpy_and_against_the_device_tables(model, name, horizon, scale):
    emu, pat, d = runs(model, name, horizon, scale)
    caps = emu.condensed_caps()
    print(caps)
    assert caps["tables_ok"] and caps["entries"] <= caps["entries_max"] == 1620 and caps["rows"] <= caps["rows_max"] == 439
    c = factored(model, name, horizon, scale)
    for k in range(horizon):
        a = check_block(emu, pat, d, k, "%s N=%d x%g" % (name, horizon, scale))
        t, glob = emu.condensed_block_through_tables(k, d["hess"], d["jac"], d["dc"], d["dx"])
        assert np.array_equal(bits(a), bits(t)), (name, horizon, k)                  # the device's tables and merge: the same bits
        diag = np.diag(unpack(a))
        assert np.array_equal(bits(c.top[NXK * k:NXK * (k + 1)]), bits(1.0 / np.maximum(np.abs(diag), FLOOR)))
        assert np.array_equal(bits(c.top[NXK * horizon:]), bits(1.0 / np.maximum(np.abs(glob), FLOOR)))
    assert np.array_equal(bits(c.bottom), bits(1.0 / d["dc"]))
    # the six globals' condensed diagonal against numpy, and their block of C is diagonal
    ir, jc = pat[2], pat[3]
    J = np.zeros((emu.m, emu.n))
    J[ir, jc] = d["jac"]
    G = J[:, NXK * horizon:]
    Cg = G.T @ (G / d["dc"][:, None])
    assert np.all(Cg[~np.eye(6, dtype=bool)] == 0.0)
    ref = d["dx"][NXK * horizon:] + np.diag(Cg)
    assert np.allclose(1.0 / c.top[NXK * horizon:], ref, rtol=64 * U, atol=0.0)


@pytest.mark.parametrize("name,horizon,lifted", [("periodic", 3, True), ("stairs", 2, True), ("single", 4, True), ("cost_ends", 2, False)])
def test_the_lifted_handle_and_other_layouts_on_synthetic_runs(model, name, horizon, lifted):
    emu, pat = emu_of(model, name, horizon, lifted)
    d = inputs(emu, 900 + horizon)
    assert emu.condensed_caps()["tables_ok"]
    for k in range(horizon):
        a = check_block(emu, pat, d, k, "%s N=%d lifted=%s" % (name, horizon, lifted))
        t, _ = emu.condensed_block_through_tables(k, d["hess"], d["jac"], d["dc"], d["dx"])
        assert np.array_equal(bits(a), bits(t)), (name, horizon, k)
    c = emu.condensed_factor(d["hess"], d["jac"], d["dc"], d["dx"], FLOOR)
    assert np.all(c.status == 0) and np.all(c.top_writes == 1) and np.all(c.bottom_writes == 1)


@pytest.mark.parametrize("name,horizon", [("periodic", 3), ("stairs", 4), ("stairs", 2)])
def test_both_jac_orders_give_the_same_bits(model, name, horizon):
    ccs, pat = emu_of(model, name, horizon)
    vf, vpat = emu_of(model, name, horizon, vary_first=True)
    d = inputs(ccs, 900 + horizon)
    at = {(int(r), int(c)): i for i, (r, c) in enumerate(zip(pat[2], pat[3]))}
    order = np.array([at[int(r), int(c)] for r, c in zip(vpat[2], vpat[3])])
    assert not np.array_equal(order, np.arange(order.size))                          # the orders do differ
    a = ccs.condensed_factor(d["hess"], d["jac"], d["dc"], d["dx"], FLOOR)
    b = vf.condensed_factor(d["hess"], d["jac"][order], d["dc"], d["dx"], FLOOR)
    for f in RECORD + ("top", "bottom"):
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y), f
    for k in range(horizon):
        t, _ = vf.condensed_block_through_tables(k, d["hess"], d["jac"][order], d["dc"], d["dx"])
        assert np.array_equal(bits(t), bits(ccs.condensed_block(k, d["hess"], d["jac"], d["dc"], d["dx"])[0])), k


@pytest.mark.parametrize("name", REAL)
def test_a_jac_run_of_zeros_gives_the_block_factorisation(model, name):
    emu, pat, d = runs(model, name, 4)
    c = emu.condensed_factor(d["hess"], np.zeros_like(d["jac"]), d["dc"], d["dx"], FLOOR)
    blk = emu.block_factor(d["hess"], d["dx"], FLOOR)
    for f in RECORD:
        assert np.array_equal(getattr(c, f), getattr(blk, f)), f                     # as numbers (-0.0 == +0.0)


# ---- 2. the factorisation and its inertia ---------------------------------------------------------------------------------------------------------
def test_factorisation_and_inertia_of_every_block(model):
    blocks = skipped = 0
    for name in REAL:
        for horizon in (2, 3, 4):
            for scale in SCALES:
                emu, pat, d = runs(model, name, horizon, scale)
                c = factored(model, name, horizon, scale)
                assert c.det_not_negative == 0 and c.not_positive_definite == 0 and np.all(c.status == 0)
                for k in range(horizon):
                    B = dense_condensed(emu, pat, d, k)[0]
                    L, D, perm, kind = split(c, k)
                    R = L @ D @ L.T - B[np.ix_(perm, perm)]
                    bound = 64 * NXK * U * np.abs(np.abs(L) @ np.abs(D) @ np.abs(L.T)).max()     # check_factorisation's
                    ev = np.linalg.eigvalsh(B)
                    print("%s N=%d x%g knot %d: |P B P^T - L D L^T|_max %.3e (bound %.3e); inertia %s, eigvalsh %s, smallest |eigenvalue| / largest %.1e"
                          % (name, horizon, scale, k, np.abs(R).max(), bound, c.inertia[k].tolist(), [(ev > 0).sum(), (ev < 0).sum()], np.abs(ev).min() / np.abs(ev).max()))
                    assert np.abs(R).max() <= bound, (name, horizon, scale, k)
                    assert c.inertia[k].sum() == NXK
                    blocks += 1
                    if np.abs(ev).min() < NXK * U * np.abs(ev).max():
                        skipped += 1
                        continue
                    assert c.inertia[k].tolist() == [int((ev > 0).sum()), int((ev < 0).sum()), 0], (name, horizon, scale, k)
    print("%d blocks, %d undecidable for the reference" % (blocks, skipped))
    assert blocks == 36 and 10 * skipped <= blocks


# ---- 3. what the inertia proves -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", REAL)
def test_dense_inertia_of_k_is_m_plus_the_negatives_of_c_which_are_at_least_a_blocks(model, name, scale):
    emu, pat, d = runs(model, name, 2, scale)
    c = factored(model, name, 2, scale)
    n, m = emu.n, emu.m
    K = kkt_check.dense(n, m, *pat[:2], d["hess"], *pat[2:], d["jac"], d["dx"], d["dc"])
    J = K[n:, :n]
    Cd = K[:n, :n] + J.T @ (J / d["dc"][:, None])
    neg_k, neg_c = int((np.linalg.eigvalsh(K) < 0).sum()), int((np.linalg.eigvalsh(Cd) < 0).sum())
    print("%s N=2 x%g: eigvalsh(K) %d negative, m = %d, neg(C) = %d, neg(B_k) = %s" % (name, scale, neg_k, m, neg_c, c.inertia[:, 1].tolist()))
    assert neg_k == m + neg_c
    assert neg_c >= int(c.inertia[:, 1].max())
    for k in range(2):                                                               # every B_k is a principal submatrix of C
        assert np.allclose(Cd[NXK * k:NXK * (k + 1), NXK * k:NXK * (k + 1)], dense_condensed(emu, pat, d, k)[0], rtol=1e-12, atol=1e-9 * np.abs(Cd).max())


# ---- 4. MINRES ------------------------------------------------------------------------------------------------------------------------------------
def minv_residual(emu, pat, d, c, sol):
    """the true residual of sol in the M^-1 norm, relative to the right-hand side's, and in the 2-norm"""
    K = kkt_check.dense(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], d["dx"], d["dc"])
    b = np.concatenate([d["bt"], d["bb"]])
    r = K @ np.concatenate([sol.top, sol.bottom]) - b

    def minv(v):
        a = emu.block_apply(c, (c.top, c.bottom), v[:emu.n], v[emu.n:])
        return np.concatenate([a.top, a.bottom])
    return float(np.sqrt(r @ minv(r)) / np.sqrt(b @ minv(b))), float(np.linalg.norm(r) / np.linalg.norm(b))


def solve_with(emu, d, rec, minv, maxiter=3000):
    return emu.block_solve(d["hess"], d["jac"], d["bt"], d["bb"], rec, minv, dx=d["dx"], dc=d["dc"], rtol=RTOL, maxiter=maxiter)


@pytest.mark.parametrize("name", REAL)
def test_real_runs_at_four_knots_converge_in_at_most_half_the_block_preconditioners_iterations(model, name):
    """seen: periodic 58 against 315, stairs 133 against 456"""
    emu, pat, d = runs(model, name, 4)
    c = factored(model, name, 4)
    sc = solve_with(emu, d, c, (c.top, c.bottom))
    blk = emu.block_factor(d["hess"], d["dx"], FLOOR)
    diag = emu.diagonal_preconditioner(d["hess"], d["jac"], d["dx"], d["dc"], FLOOR)
    sb = solve_with(emu, d, blk, (diag.top, diag.bottom))
    true_m, true_2 = minv_residual(emu, pat, d, c, sc)
    print("%s N=4 U[1,2]: condensed status %d after %d iterations, residual %.3e, true %.3e in the M^-1 norm (%.3e in the 2-norm); block status %d after %d"
          % (name, sc.status, sc.iterations, sc.residual, true_m, true_2, sb.status, sb.iterations))
    assert sc.status == 0 and sb.status == 0
    assert 2 * sc.iterations <= sb.iterations
    assert true_m <= 100.0 * RTOL
    assert np.all(sc.top_writes >= 1) and np.all(sc.bottom_writes >= 1)


@pytest.mark.parametrize("name,horizon", [("periodic", 4), ("stairs", 4), ("periodic", 2)])
def test_with_small_diagonals_it_converges_where_the_block_preconditioner_does_not(model, name, horizon):
    """dx, dc multiplied by 1e-4; seen: 247, 340 and 155 iterations, block_preconditioner status 1 after 3 000"""
    emu, pat, d = runs(model, name, horizon, 1e-4)
    c = factored(model, name, horizon, 1e-4)
    sc = solve_with(emu, d, c, (c.top, c.bottom))
    blk = emu.block_factor(d["hess"], d["dx"], FLOOR)
    diag = emu.diagonal_preconditioner(d["hess"], d["jac"], d["dx"], d["dc"], FLOOR)
    sb = solve_with(emu, d, blk, (diag.top, diag.bottom))
    true_m, true_2 = minv_residual(emu, pat, d, c, sc)
    print("%s N=%d x1e-4: condensed status %d after %d iterations, residual %.3e, true %.3e in the M^-1 norm (%.3e in the 2-norm); block status %d after %d, residual %.3e"
          % (name, horizon, sc.status, sc.iterations, sc.residual, true_m, true_2, sb.status, sb.iterations, sb.residual))
    assert sc.status == 0 and sc.iterations <= 3000
    assert true_m <= 100.0 * RTOL
    assert (sb.status, sb.iterations) == (1, 3000)


@pytest.mark.parametrize("name", REAL)
def test_the_diagonal_the_launch_writes_is_a_preconditioner_on_its_own(model, name):
    """status 0 implies the true residual in ITS M^-1 norm within 100 rtol; no count is asserted (seen: 538 and 988 at N = 4, U[1, 2])"""
    emu, pat, d = runs(model, name, 4)
    c = factored(model, name, 4)
    s = emu.solve(d["hess"], d["jac"], d["bt"], d["bb"], dx=d["dx"], dc=d["dc"], minv=(c.top, c.bottom), rtol=RTOL, maxiter=3000)
    K = kkt_check.dense(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], d["dx"], d["dc"])
    b, w = np.concatenate([d["bt"], d["bb"]]), np.concatenate([c.top, c.bottom])
    r = K @ np.concatenate([s.top, s.bottom]) - b
    true_m = float(np.sqrt(r @ (w * r)) / np.sqrt(b @ (w * b)))
    print("%s N=4 condensed diagonal alone: status %d after %d iterations, residual %.3e, true %.3e in the M^-1 norm" % (name, s.status, s.iterations, s.residual, true_m))
    assert np.all(w > 0.0)
    if s.status == 0:
        assert true_m <= 100.0 * RTOL


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------------------------------
def knots_of_row(pat, i, horizon):
    """the knots whose column block holds row i of g"""
    ir, jc = pat[2], pat[3]
    cols = jc[(ir == i) & (jc < NXK * horizon)]
    return sorted(set((cols // NXK).tolist()))


def same_knot(a, b, k):
    return all(np.array_equal(bits(getattr(a, f)[k]) if getattr(a, f).dtype == np.float64 else getattr(a, f)[k],
                              bits(getattr(b, f)[k]) if getattr(b, f).dtype == np.float64 else getattr(b, f)[k]) for f in RECORD)


def is_nan_record(c, k):
    return c.status[k] == 2 and c.inertia[k].tolist() == [0, 0, 0] and np.all(np.isnan(c.factor[k])) and np.all(np.isnan(c.e[k])) and np.all(np.isnan(c.o[k]))


def no_sentinel_left(c):
    assert np.all(c.top_writes == 1) and np.all(c.bottom_writes == 1)
    for f in ("factor", "e", "o", "top", "bottom"):
        assert not np.any(getattr(c, f) == -7.0), f
    assert not np.any(c.words == -99) and not np.any(c.inertia == -99) and not np.any(c.status == -99)


@pytest.mark.parametrize("name,horizon", [("stairs", 4), ("periodic", 2)])
def test_a_nan_in_one_knots_hessian_gives_status_2_for_that_knot_only(model, name, horizon):
    emu, pat, d = runs(model, name, horizon)
    clean = factored(model, name, horizon)
    nnz_knot = emu.block_pattern()[1].size
    hess = d["hess"].copy()
    bad = horizon - 1
    hess[bad * nnz_knot + 5] = np.nan
    c = emu.condensed_factor(hess, d["jac"], d["dc"], d["dx"], FLOOR)
    no_sentinel_left(c)
    assert c.status.tolist() == [2 if k == bad else 0 for k in range(horizon)] and is_nan_record(c, bad)
    for k in range(horizon):
        if k != bad:
            assert same_knot(c, clean, k)
    assert not np.any(np.isnan(c.bottom))
    sol = solve_with(emu, d, c, (c.top, c.bottom), maxiter=5)
    assert (sol.status, sol.iterations) == (2, 0)


@pytest.mark.parametrize("value", [0.0, -1.5, float("nan"), float("inf")])
@pytest.mark.parametrize("name,horizon", [("periodic", 4), ("stairs", 3), ("periodic", 2)])
def test_a_bad_dc_gives_status_2_for_exactly_the_knots_whose_column_block_holds_the_row(model, name, horizon, value):
    emu, pat, d = runs(model, name, horizon)
    clean = factored(model, name, horizon)
    sets = {i: tuple(knots_of_row(pat, i, horizon)) for i in range(emu.m)}
    wanted = [(k,) for k in range(horizon)] + [(k, k + 1) for k in range(horizon - 1)] + ([(0, horizon - 1)] if name == "periodic" and horizon > 2 else [])
    rows = [next(i for i in range(emu.m) if sets[i] == w) for w in wanted if w in sets.values()]
    assert len(rows) >= horizon + 1                                                  # rows inside one knot, and rows that touch two
    for i in rows:
        dc = d["dc"].copy()
        dc[i] = value
        c = emu.condensed_factor(d["hess"], d["jac"], dc, d["dx"], FLOOR)
        no_sentinel_left(c)
        assert c.status.tolist() == [2 if k in sets[i] else 0 for k in range(horizon)], (i, sets[i])
        for k in range(horizon):
            assert is_nan_record(c, k) if k in sets[i] else same_knot(c, clean, k), (i, k)
        assert np.isnan(c.bottom[i]) and np.count_nonzero(np.isnan(c.bottom)) == 1
