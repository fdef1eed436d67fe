"""The diagonal preconditioner of the KKT solve (hippopt_amd/csrc/knot_kkt_precond.h), built by the CPU emulation of
hipnlp_kkt_diag_precond_device (tests/kkt_precond_emu):

    minv_top_j = 1 / max(|H_jj + dx_j|, floor),     minv_bottom_i = 1 / max(|dc_i + sum_e J_ie^2 minv_top_col(e)|, floor)

against a numpy restatement through the two patterns, the stores, both jac orders, omitted diagonals, the floor, NaN and infinity; then
what it is for: on symmetrically rescaled systems K' = S K S (S = diag 10^U(-3, 3): cond about 1e12) MINRES with the built diagonal converges
in the iteration count of the unscaled system where the identity does not converge at all, and on the real N = 4 value runs of the stairs
terrain it is the difference between status 0 and status 1 at 3000 iterations.

Measured with this emulation (rtol 1e-8): rescaled periodic N=2 / cost_ends N=3 / stairs N=3 / single N=4 lifted: status 0 after 23 / 25 / 25 /
25 iterations, the same counts unscaled, identity status 1 at 300 with residuals of 4.2e-2 to 5.5e-2.  Real stairs N=4: built status 0 after
2194 iterations (a numpy-built diagonal: 2191), identity status 1 at 3000 with residual 0.47.  CPU only."""
import numpy as np
import pytest

import kkt_check
from hvp_check import gamma
from kkt_check import bits
from kkt_emu_lib import NXK
from test_kkt_minres_hostemu import inputs
from test_lagrangian_grad_hostemu import MAKERS

SMALL = [(name, horizon) for name in MAKERS for horizon in (2, 3, 4)]      # N = 4: all four pair variants; N = 2: first and last only
BOTH_ORDERS = [("periodic", 3), ("cost_ends", 2)]
RESCALED = [("periodic", 2, False), ("cost_ends", 3, False), ("stairs", 3, False), ("single", 4, True)]
FLOOR = 1e-10
_EMU, _BUILT = {}, {}


def emu_of(model, name, horizon, lifted, vary_first=False):
    from kkt_precond_emu_lib import KktPrecondEmu
    key = (name, horizon, lifted, vary_first)
    if key not in _EMU:
        emu = KktPrecondEmu(MAKERS[name](horizon, model), model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
        _EMU[key] = (emu, tuple(np.asarray(a) for a in emu.hess_sparsity() + emu.sparsity()))
    return _EMU[key]


def built(model, name, horizon, lifted, vary_first=False):
    """(emulation, patterns, inputs, Diagonal) on the conditioned inputs of tests/test_kkt_minres_hostemu.py, computed once"""
    key = (name, horizon, lifted, vary_first)
    if key not in _BUILT:
        emu, pat = emu_of(model, name, horizon, lifted, vary_first)
        d = inputs(emu, 900 + horizon)
        _BUILT[key] = (emu, pat, d, emu.diagonal_preconditioner(d["hess"], d["jac"], d["dx"], d["dc"], FLOOR))
    return _BUILT[key]


def hess_diagonal(pat, hess, n):
    """diag H through the pattern (+0.0 where it has no entry), and the entry's index in the value run (-1: none)"""
    hr, hc = pat[:2]
    on = np.flatnonzero(hr == hc)
    assert np.unique(hr[on]).size == on.size                                # at most one diagonal entry per variable
    hd, where = np.zeros(n), np.full(n, -1)
    hd[hr[on]], where[hr[on]] = hess[on], on
    return hd, where


def numpy_diagonal(emu, pat, hess, jac, dx, dc, floor):
    """(top, bottom, entries per row): top in float64 (one add, one abs, one division: the same operations); the row sums of bottom in
    long double, so that the reference's own rounding is far below the bound of the float64 chain it is compared with"""
    ir, jc = pat[2:]
    hd, _ = hess_diagonal(pat, hess, emu.n)
    top = 1.0 / np.maximum(np.abs(hd + dx if dx is not None else hd), floor)
    s = np.zeros(emu.m, np.longdouble)
    np.add.at(s, ir, np.asarray(jac, np.longdouble) ** 2 * np.asarray(top, np.longdouble)[jc])
    if dc is not None:
        s = s + np.asarray(dc, np.longdouble)
    return top, np.asarray(1.0 / np.maximum(np.abs(s), np.longdouble(floor)), np.float64), np.bincount(ir, minlength=emu.m)


def assert_against_numpy(emu, pat, hess, jac, dx, dc, got, what, floor=FLOOR):
    top, bottom, k = numpy_diagonal(emu, pat, hess, jac, dx, dc, floor)
    err_t = np.abs(got.top - top) / np.spacing(top)
    err_b = np.abs(got.bottom - bottom) / bottom
    bound = gamma(k + 3)                                                     # k + 1 non-negative terms and the division
    print("%s: minv_top within %.1f ulp, minv_bottom within %.3f of gamma(k + 3) (rows of up to %d entries)" % (what, err_t.max(), (err_b / bound).max(), k.max()))
    assert np.all(err_t <= 2.0), np.flatnonzero(err_t > 2.0)[:8]
    assert np.all(err_b <= bound), np.flatnonzero(err_b > bound)[:8]
    assert np.all(got.top > 0.0) and np.all(got.bottom > 0.0)


def matrix(cases, orders=False):
    def deco(fn):
        marks = [pytest.mark.parametrize("name,horizon", cases), pytest.mark.parametrize("lifted", [False, True])]
        if orders:
            marks.append(pytest.mark.parametrize("vary_first", [False, True]))
        for mark in marks:
            fn = mark(fn)
        return fn
    return deco


# ---- 1. against numpy, the stores ---------------------------------------------------------------------------------------------------------------
@matrix(SMALL)
def test_against_numpy_and_every_element_is_stored_once(model, name, horizon, lifted):
    emu, pat, d, got = built(model, name, horizon, lifted)
    assert_against_numpy(emu, pat, d["hess"], d["jac"], d["dx"], d["dc"], got, "%s N=%d lifted=%s" % (name, horizon, lifted))
    assert got.top_writes.shape == (emu.n,) and got.bottom_writes.shape == (emu.m,)
    assert np.all(got.top_writes == 1), np.flatnonzero(got.top_writes != 1)[:8]
    assert np.all(got.bottom_writes == 1), np.flatnonzero(got.bottom_writes != 1)[:8]


@matrix(SMALL)
def test_the_diagonal_positions_are_those_of_the_pattern(model, name, horizon, lifted):
    """HessLayout's new table against hess_sparsity(): the same entry for every knot, -1 exactly where the pattern has no diagonal entry"""
    emu, pat = emu_of(model, name, horizon, lifted)
    pos = emu.diag_positions()
    _, where = hess_diagonal(pat, np.zeros(emu.nnz_h), emu.n)
    nnz_knot = (emu.nnz_h - np.count_nonzero(pat[0] // NXK != pat[1] // NXK)) // horizon     # (without the periodicity coupling behind the blocks)
    for k in range(horizon):
        for i in range(NXK):
            assert where[NXK * k + i] == (nnz_knot * k + pos[i] if pos[i] >= 0 else -1), (k, i)
    assert np.all(where[NXK * horizon:] == -1)                       # no entry touches a horizon-global variable


@matrix(BOTH_ORDERS)
def test_both_jac_orders_give_the_same_bits(model, name, horizon, lifted):
    emu, pat, d, got = built(model, name, horizon, lifted)
    other, opat = emu_of(model, name, horizon, lifted, vary_first=True)
    assert not np.array_equal(pat[2], opat[2]) or not np.array_equal(pat[3], opat[3])
    here, there = np.argsort(pat[2].astype(np.int64) * emu.n + pat[3], kind="stable"), np.argsort(opat[2].astype(np.int64) * emu.n + opat[3], kind="stable")
    jac = np.empty_like(d["jac"])
    jac[there] = d["jac"][here]                                               # the same matrix in the other order of the value run
    twin = other.diagonal_preconditioner(d["hess"], jac, d["dx"], d["dc"], FLOOR)
    assert np.array_equal(bits(twin.top), bits(got.top)) and np.array_equal(bits(twin.bottom), bits(got.bottom))
    assert np.all(twin.top_writes == 1) and np.all(twin.bottom_writes == 1)


@pytest.mark.parametrize("diagonals", [(False, False), (True, False), (False, True)])
@matrix(SMALL)
def test_omitted_diagonals(model, name, horizon, lifted, diagonals):
    """dx, dc or both left out: |H_jj| alone is tiny or zero where the random pattern value is, so the floor is at work here too"""
    emu, pat, d, full = built(model, name, horizon, lifted)
    dx, dc = d["dx"] if diagonals[0] else None, d["dc"] if diagonals[1] else None
    got = emu.diagonal_preconditioner(d["hess"], d["jac"], dx, dc, FLOOR)
    assert_against_numpy(emu, pat, d["hess"], d["jac"], dx, dc, got, "%s N=%d lifted=%s diagonals=%s" % (name, horizon, lifted, diagonals))
    assert np.all(got.top_writes == 1) and np.all(got.bottom_writes == 1)
    assert not np.array_equal(bits(got.bottom), bits(full.bottom))
    if not diagonals[0]:
        assert np.all(got.top[emu.n - 6:] == 1.0 / FLOOR)                     # the six globals: no Hessian entry and no dx


# ---- 2. the floor, NaN and infinity ----------------------------------------------------------------------------------------------------------------
def chosen_columns(emu, pat, horizon):
    """a column of a row's own record, one of its predecessor's record, a horizon-global one and, where a row couples both horizon ends,
    one of the other end's record: (row, column) each"""
    ir, jc = pat[2:]
    knots = np.minimum(jc // NXK, horizon)                                     # (horizon: the globals)
    span = {}
    for r, kn, c in zip(ir, knots, jc):
        span.setdefault(int(r), {}).setdefault(int(kn), int(c))
    two = next(r for r, s in sorted(span.items()) if len([q for q in s if q < horizon]) == 2 and max(q for q in s if q < horizon) - min(s) == 1)
    glob = next((r for r, s in sorted(span.items()) if horizon in s), None)        # (a layout may leave the global columns of jac g empty)
    low, high = sorted(q for q in span[two] if q < horizon)
    picks = [(two, span[two][high]), (two, span[two][low]), (glob, span[glob][horizon] if glob is not None else NXK * horizon)]
    ends = next((r for r, s in sorted(span.items()) if horizon > 2 and 0 in s and horizon - 1 in s), None)
    if ends is not None:
        picks.append((ends, span[ends][0]))                                      # a periodicity row: owned by the last knot, column at the other end
    return picks


@matrix([("periodic", 2), ("cost_ends", 3), ("stairs", 4), ("single", 4)])
def test_the_floor_is_exact(model, name, horizon, lifted):
    emu, pat, d, clean = built(model, name, horizon, lifted)
    ir, jc = pat[2:]
    _, where = hess_diagonal(pat, d["hess"], emu.n)
    picks = chosen_columns(emu, pat, horizon)
    assert picks[0][1] // NXK == picks[1][1] // NXK + 1 and picks[2][1] >= NXK * horizon
    hess, dx = d["hess"].copy(), d["dx"].copy()
    for _, c in picks:
        if where[c] >= 0:
            hess[where[c]] = 0.0
        dx[c] = 0.0
    for floor in (FLOOR, 0.25):
        got = emu.diagonal_preconditioner(hess, d["jac"], dx, d["dc"], floor)
        for _, c in picks:
            assert got.top[c] == 1.0 / floor, (c, got.top[c])
        assert_against_numpy(emu, pat, hess, d["jac"], dx, d["dc"], got, "%s N=%d floor=%g" % (name, horizon, floor), floor)
    cols = np.array([c for _, c in picks])
    same_t, same_b = np.setdiff1d(np.arange(emu.n), cols), np.setdiff1d(np.arange(emu.m), ir[np.isin(jc, cols)])
    got = emu.diagonal_preconditioner(hess, d["jac"], dx, d["dc"], FLOOR)
    assert np.array_equal(bits(got.top[same_t]), bits(clean.top[same_t])) and np.array_equal(bits(got.bottom[same_b]), bits(clean.bottom[same_b]))
    for r, _ in picks:
        assert r is None or got.bottom[r] < clean.bottom[r]                      # a term J^2 / floor more in the sum
    # the bottom: a row without entries that count and without dc
    r = picks[0][0]
    jac, dc = d["jac"].copy(), d["dc"].copy()
    jac[ir == r], dc[r] = 0.0, 0.0
    got = emu.diagonal_preconditioner(d["hess"], jac, d["dx"], dc, FLOOR)
    assert got.bottom[r] == 1.0 / FLOOR
    rest = np.arange(emu.m) != r
    assert np.array_equal(bits(got.bottom[rest]), bits(clean.bottom[rest])) and np.array_equal(bits(got.top), bits(clean.top))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@matrix([("periodic", 2), ("cost_ends", 3), ("stairs", 4), ("single", 4)])
def test_a_value_that_is_not_finite_surfaces_where_it_is_used_and_nowhere_else(model, name, horizon, lifted, bad):
    """not clamped away by the floor, and 1 / inf = 0 does not hide an infinity: NaN in exactly the outputs that depend on the value"""
    emu, pat, d, clean = built(model, name, horizon, lifted)
    ir, jc = pat[2:]
    _, where = hess_diagonal(pat, d["hess"], emu.n)

    def check(got, cols, rows, what):
        t, b = np.zeros(emu.n, bool), np.zeros(emu.m, bool)
        t[cols], b[rows] = True, True
        assert np.all(np.isnan(got.top[t])) and np.all(np.isnan(got.bottom[b])), what
        assert np.array_equal(bits(got.top[~t]), bits(clean.top[~t])) and np.array_equal(bits(got.bottom[~b]), bits(clean.bottom[~b])), what
        assert np.all(got.top_writes == 1) and np.all(got.bottom_writes == 1)

    for _, c in chosen_columns(emu, pat, horizon):                                # own, predecessor's, global: recomputed by the row's owner
        hess, dx = d["hess"].copy(), d["dx"].copy()
        if where[c] >= 0:
            hess[where[c]] = bad
        else:
            dx[c] = bad
        rows = np.unique(ir[jc == c])
        assert rows.size > 0 or c >= NXK * horizon
        check(emu.diagonal_preconditioner(hess, d["jac"], dx, d["dc"], FLOOR), [c], rows, ("hess / dx of column", c))
    off = int(np.flatnonzero(pat[0] != pat[1])[0])
    hess = d["hess"].copy()
    hess[off] = bad
    check(emu.diagonal_preconditioner(hess, d["jac"], d["dx"], d["dc"], FLOOR), [], [], "an off-diagonal entry of the Hessian is not read")
    for e in (0, emu.nnz // 2, emu.nnz - 1):
        jac = d["jac"].copy()
        jac[e] = bad
        check(emu.diagonal_preconditioner(d["hess"], jac, d["dx"], d["dc"], FLOOR), [], [ir[e]], ("jac entry", e))
    dc = d["dc"].copy()
    dc[emu.m // 2] = bad
    check(emu.diagonal_preconditioner(d["hess"], d["jac"], d["dx"], dc, FLOOR), [], [emu.m // 2], "dc")
    bt, bb = d["bt"], d["bb"]
    hess = d["hess"].copy()
    hess[where[where >= 0][0]] = bad
    got = emu.diagonal_preconditioner(hess, d["jac"], d["dx"], d["dc"], FLOOR)
    sol = emu.solve(d["hess"], d["jac"], bt, bb, dx=d["dx"], dc=d["dc"], minv=(got.top, got.bottom), maxiter=5)
    assert (sol.status, sol.iterations) == (2, 0)                                # the solve reports such a diagonal as a breakdown


# ---- 3. scale invariance and convergence ----------------------------------------------------------------------------------------------------------
def rescaled(emu, pat, horizon):
    """(inputs, rescaled inputs, s_top, s_bot): K' = S K S, b' = S b, S = diag(s_top, s_bot) = 10^U(-3, 3)"""
    hr, hc, ir, jc = pat
    d = inputs(emu, 900 + horizon)
    rng = np.random.RandomState(1900 + horizon)
    s_top = 10.0 ** rng.uniform(-3.0, 3.0, emu.n)
    s_bot = 10.0 ** rng.uniform(-3.0, 3.0, emu.m)
    r = dict(hess=d["hess"] * s_top[hr] * s_top[hc], jac=d["jac"] * s_bot[ir] * s_top[jc], dx=d["dx"] * s_top ** 2, dc=d["dc"] * s_bot ** 2, bt=d["bt"] * s_top, bb=d["bb"] * s_bot)
    return d, r, s_top, s_bot


def true_residual(emu, pat, d, sol, minv):
    """sqrt(r . M^-1 r) / sqrt(b . M^-1 b), r = b - K z through the patterns in float64"""
    kt, kb = kkt_check.apply(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], d["dx"], d["dc"], sol.top, sol.bottom)
    r, b, mi = np.concatenate([d["bt"] - kt, d["bb"] - kb]), np.concatenate([d["bt"], d["bb"]]), np.concatenate(minv)
    return float(np.sqrt(np.dot(r, mi * r)) / np.sqrt(np.dot(b, mi * b)))


@pytest.mark.parametrize("name,horizon,lifted", RESCALED)
def test_rescaled_systems_converge_with_the_built_diagonal_and_not_without(model, name, horizon, lifted):
    emu, pat = emu_of(model, name, horizon, lifted)
    d, r, s_top, s_bot = rescaled(emu, pat, horizon)
    K = kkt_check.dense(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], d["dx"], d["dc"])
    Kr = kkt_check.dense(emu.n, emu.m, *pat[:2], r["hess"], *pat[2:], r["jac"], r["dx"], r["dc"])
    cond, cond_r = float(np.linalg.cond(K)), float(np.linalg.cond(Kr))
    plain = emu.diagonal_preconditioner(d["hess"], d["jac"], d["dx"], d["dc"], FLOOR)
    diag = emu.diagonal_preconditioner(r["hess"], r["jac"], r["dx"], r["dc"], FLOOR)
    assert np.all(diag.top_writes == 1) and np.all(diag.bottom_writes == 1)
    base = emu.solve(d["hess"], d["jac"], d["bt"], d["bb"], dx=d["dx"], dc=d["dc"], minv=(plain.top, plain.bottom), rtol=1e-8, maxiter=100)
    sol = emu.solve(r["hess"], r["jac"], r["bt"], r["bb"], dx=r["dx"], dc=r["dc"], minv=(diag.top, diag.bottom), rtol=1e-8, maxiter=100)
    ident = emu.solve(r["hess"], r["jac"], r["bt"], r["bb"], dx=r["dx"], dc=r["dc"], rtol=1e-8, maxiter=300)
    true = true_residual(emu, pat, r, sol, (diag.top, diag.bottom))
    ref = np.linalg.solve(K, np.concatenate([d["bt"], d["bb"]]))
    err = float(np.linalg.norm(np.concatenate([sol.top * s_top, sol.bottom * s_bot]) - ref) / np.linalg.norm(ref))
    print("%s N=%d lifted=%s: cond(K) %.2f, cond(S K S) %.2e; built: status %d after %d iterations (unscaled: %d), residual %.3e (true %.3e), unscaled error %.3e "
          "(bound %.3e); identity: status %d after %d, residual %.3e"
          % (name, horizon, lifted, cond, cond_r, sol.status, sol.iterations, base.iterations, sol.residual, true, err, cond * 2e-8, ident.status, ident.iterations, ident.residual))
    assert cond_r > 1e8 * cond
    assert sol.status == 0 and 0 < sol.iterations <= 100
    assert true <= 2e-8
    assert err <= cond * 2.0 * 1e-8
    assert (ident.status, ident.iterations) == (1, 300)
    assert base.status == 0 and abs(sol.iterations - base.iterations) <= 2          # M'^-1/2 K' M'^-1/2 = M^-1/2 K M^-1/2 in exact arithmetic


# ---- 4. real value runs ------------------------------------------------------------------------------------------------------------------------------
def test_real_value_runs_on_the_stairs_converge_with_the_built_diagonal_and_not_without(model):
    """the N = 4 workload of tests/test_gpu_kkt_minres.py's real-runs test, trajectory 0: max |H| 4.4e7, 21 negative diagonals of H + dx,
    cond(K) 3.2e9.  Nothing here makes an interior-point step cheap: about 2200 iterations for 1445 unknowns."""
    from hippopt_amd.synthetic import make_workload, place_on_step_flanks
    from hostemu_lib import HostEmu
    from hvp_emu_lib import HvpEmu
    st = MAKERS["stairs"](4, model)
    x, p = make_workload(st, model, batch=1, seed=8900)
    place_on_step_flanks(x[:1], st, seed=3)
    emu, pat = emu_of(model, "stairs", 4, False)
    rng = np.random.RandomState(11)
    lam, dx, dc = rng.standard_normal(emu.m), rng.uniform(1.0, 2.0, emu.n), rng.uniform(1.0, 2.0, emu.m)
    bt, bb = rng.standard_normal(emu.n), rng.standard_normal(emu.m)
    hess = HvpEmu(st, model).hess_vec(x[0], p[0], 0.8, lam, np.zeros(emu.n), want_values=True)[2]
    jac = HostEmu(st, model).eval(x[0], p[0])[3]
    diag = emu.diagonal_preconditioner(hess, jac, dx, dc, FLOOR)
    assert_against_numpy(emu, pat, hess, jac, dx, dc, diag, "stairs N=4 real value runs")
    hd, _ = hess_diagonal(pat, hess, emu.n)
    sol = emu.solve(hess, jac, bt, bb, dx=dx, dc=dc, minv=(diag.top, diag.bottom), rtol=1e-8, maxiter=3000)
    ident = emu.solve(hess, jac, bt, bb, dx=dx, dc=dc, rtol=1e-8, maxiter=3000)
    print("stairs N=4 real value runs: |hess| up to %.2e, %d negative diagonals of H + dx; built: status %d after %d iterations, residual %.3e; identity: status %d after %d, "
          "residual %.3e" % (np.abs(hess).max(), int(np.count_nonzero(hd + dx < 0.0)), sol.status, sol.iterations, sol.residual, ident.status, ident.iterations, ident.residual))
    assert np.count_nonzero(hd + dx < 0.0) > 0                                       # the absolute value is at work
    assert sol.status == 0 and sol.iterations <= 3000 and sol.residual <= 1e-8
    assert (ident.status, ident.iterations) == (1, 3000)
