"""Preconditioned MINRES on the one-launch KKT operator (hippopt_amd/csrc/knot_minres.h), run by the CPU emulation of
hipnlp_kkt_minres_device (tests/kkt_minres_emu) on CONDITIONED random value runs: 0.05 standard_normal for both runs, dx, dc in U[1, 2],
b standard normal (cond(K) about 3 to 5; nothing here says anything about the KKT systems of real iterates).  Convergence to rtol 1e-8 and
1e-12 with and without a diagonal preconditioner in U[0.5, 2], the true residual against the estimate, the solution against a dense solve,
the two dot products of every iteration against numpy within the rounding bound of their sums, freezing, the iteration limit, b = 0, a
preconditioner that is not positive definite, the stores to the six outputs, and omitted diagonals (dx, dc or both: K is then singular on
these value runs, so 25 iterations are checked sum by sum and by their true residual, not by convergence).  CPU only."""
import numpy as np
import pytest

import kkt_check
from hvp_check import gamma, touch_counts
from kkt_check import bits
from test_lagrangian_grad_hostemu import MAKERS

SMALL = [(name, horizon) for name in MAKERS for horizon in (2, 3, 4)]
CASES = SMALL + [("periodic", 30)]
BOTH_ORDERS = [("periodic", 3), ("cost_ends", 2)]
RTOLS = (1e-8, 1e-12)
MAXITER = {False: 100, True: 300}       # without / with minv: about 30 % over the largest count of a numpy restatement on these inputs
_EMU, _SOL = {}, {}


def emu_of(model, name, horizon, lifted, vary_first=False):
    from kkt_minres_emu_lib import KktMinresEmu
    key = (name, horizon, lifted, vary_first)
    if key not in _EMU:
        emu = KktMinresEmu(MAKERS[name](horizon, model), model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
        _EMU[key] = (emu, emu.hess_sparsity() + emu.sparsity())
    return _EMU[key]


def inputs(emu, seed):
    rng = np.random.RandomState(seed)
    return dict(hess=0.05 * rng.standard_normal(emu.nnz_h), jac=0.05 * rng.standard_normal(emu.nnz), dx=rng.uniform(1.0, 2.0, emu.n), dc=rng.uniform(1.0, 2.0, emu.m),
                bt=rng.standard_normal(emu.n), bb=rng.standard_normal(emu.m), mt=rng.uniform(0.5, 2.0, emu.n), mb=rng.uniform(0.5, 2.0, emu.m))


def solve(model, name, horizon, lifted, vary_first=False, rtol=1e-8, with_minv=False, maxiter=None, diagonals=(True, True), **kw):
    """(emulation, patterns, inputs, Solution), computed once per argument set; diagonals: whether dx / dc are passed (d["dx"] / d["dc"]
    of the returned inputs are None for an omitted one)"""
    key = (name, horizon, lifted, vary_first, rtol, with_minv, maxiter, diagonals, tuple(sorted(kw.items())))
    if key not in _SOL:
        emu, pat = emu_of(model, name, horizon, lifted, vary_first)
        d = inputs(emu, 900 + horizon)
        d["dx"], d["dc"] = d["dx"] if diagonals[0] else None, d["dc"] if diagonals[1] else None
        sol = emu.solve(d["hess"], d["jac"], d["bt"], d["bb"], dx=d["dx"], dc=d["dc"], minv=(d["mt"], d["mb"]) if with_minv else None, rtol=rtol,
                        maxiter=MAXITER[with_minv] if maxiter is None else maxiter, **kw)
        _SOL[key] = (emu, pat, d, sol)
    return _SOL[key]


def true_residual(emu, pat, d, sol, with_minv):
    """sqrt(r . M^-1 r) / sqrt(b . M^-1 b), r = b - K z through the patterns in float64"""
    kt, kb = kkt_check.apply(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], d["dx"], d["dc"], sol.top, sol.bottom)
    r, b = np.concatenate([d["bt"] - kt, d["bb"] - kb]), np.concatenate([d["bt"], d["bb"]])
    mi = np.concatenate([d["mt"], d["mb"]]) if with_minv else np.ones(emu.n + emu.m)
    return float(np.sqrt(np.dot(r, mi * r)) / np.sqrt(np.dot(b, mi * b)))


def matrix(cases, orders=False):
    def deco(fn):
        marks = [pytest.mark.parametrize("name,horizon", cases), pytest.mark.parametrize("lifted", [False, True])]
        if orders:
            marks.append(pytest.mark.parametrize("vary_first", [False, True]))
        for mark in marks:
            fn = mark(fn)
        return fn
    return deco


# ---- 1. convergence -------------------------------------------------------------------------------------------------------------------------
def converges(model, name, horizon, lifted, vary_first, rtol, with_minv):
    emu, pat, d, sol = solve(model, name, horizon, lifted, vary_first, rtol, with_minv)
    true = true_residual(emu, pat, d, sol, with_minv)
    print("%s N=%d lifted=%s vary_first=%s rtol=%g minv=%s: status %d after %d iterations, residual %.3e (true %.3e)"
          % (name, horizon, lifted, vary_first, rtol, with_minv, sol.status, sol.iterations, sol.residual, true))
    assert sol.status == 0 and 0 < sol.iterations <= MAXITER[with_minv]
    assert sol.residual <= rtol and true <= 2.0 * rtol and abs(sol.residual - true) <= rtol


@pytest.mark.parametrize("with_minv", [False, True])
@pytest.mark.parametrize("rtol", RTOLS)
@matrix(CASES)
def test_converges_and_the_estimate_is_the_true_residual(model, name, horizon, lifted, rtol, with_minv):
    converges(model, name, horizon, lifted, False, rtol, with_minv)


@pytest.mark.parametrize("with_minv", [False, True])
@matrix(BOTH_ORDERS, orders=True)
def test_converges_in_both_jac_orders(model, name, horizon, lifted, vary_first, with_minv):
    converges(model, name, horizon, lifted, vary_first, 1e-8, with_minv)


# ---- 2. against a dense solve ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_minv", [False, True])
@pytest.mark.parametrize("rtol", RTOLS)
@matrix(SMALL)
def test_solution_against_a_dense_solve(model, name, horizon, lifted, rtol, with_minv):
    emu, pat, d, sol = solve(model, name, horizon, lifted, False, rtol, with_minv)
    K = kkt_check.dense(emu.n, emu.m, *pat[:2], d["hess"], *pat[2:], d["jac"], d["dx"], d["dc"])
    ref = np.linalg.solve(K, np.concatenate([d["bt"], d["bb"]]))
    cond = float(np.linalg.cond(K))
    err = float(np.linalg.norm(np.concatenate([sol.top, sol.bottom]) - ref) / np.linalg.norm(ref))
    print("%s N=%d lifted=%s rtol=%g minv=%s: cond(K) %.2f, relative error %.3e (bound %.3e)" % (name, horizon, lifted, rtol, with_minv, cond, err, cond * 2.0 * rtol))
    assert err <= cond * 2.0 * rtol


# ---- 3. the dot products of every iteration ---------------------------------------------------------------------------------------------------
def alfa_and_beta_against_numpy(model, name, horizon, lifted, with_minv, diagonals=(True, True), maxiter=None):
    """A plain numpy restatement of one iteration from the emulation's own v, r1 and r2 (a restatement that ran on its own would drift
    away along the Krylov sequence and say nothing about one sum):
        y = K v - (beta/oldb) r1 through the patterns in float64, every element within 2 gamma_{k_max + 1} (|K| |v| + |c1 r1|)_e;
        alfa = v . y within 2 gamma_{n + m + k_max} |v| . (|K| |v| + |c1 r1|) — the bound of tests/test_kkt_operator_hostemu.py, k_max the
        longest sum of an element of K v, the diagonal counted;
        beta^2 = r2 . M^-1 r2 from the emulation's new r2: within 2 gamma_{n + m + 1} |r2| . |M^-1 r2| + 4 * 2^-53 beta^2 (the square root and
        squaring it back round three times).
    Returns (emulation, patterns, inputs, Solution)."""
    emu, pat, d, sol = solve(model, name, horizon, lifted, False, 1e-8, with_minv, maxiter=maxiter, diagonals=diagonals, trace=True, trace_vec=True)
    n, m = emu.n, emu.m
    hr, hc, ir, jc = pat
    k_max = max(int((touch_counts(hr, hc, n) + np.bincount(jc, minlength=n)).max()), int(np.bincount(ir, minlength=m).max())) + 1
    b = np.concatenate([d["bt"], d["bb"]])
    mi = np.concatenate([d["mt"], d["mb"]]) if with_minv else np.ones(n + m)
    assert sol.iterations >= 10
    beta = [float(np.sqrt(np.dot(b, mi * b)))] + list(sol.trace[:, 1])
    worst_a = worst_b = 0.0
    for it in range(1, sol.iterations + 1):
        alfa, beta_new, _, _, count, ran = sol.trace[it - 1]
        assert ran == 1.0 and count == it
        v, y, r2n, ym = sol.trace_vec[it - 1]
        r1 = b if it == 2 else (sol.trace_vec[it - 3][2] if it > 2 else np.zeros(n + m))
        c1 = beta[it - 1] / beta[it - 2] if it >= 2 else 0.0
        kt, kb = kkt_check.apply(n, m, hr, hc, d["hess"], ir, jc, d["jac"], d["dx"], d["dc"], v[:n], v[n:])
        at, ab = kkt_check.apply(n, m, hr, hc, d["hess"], ir, jc, d["jac"], d["dx"], d["dc"], v[:n], v[n:], absolute=True)
        y_np = np.concatenate([kt, kb]) - c1 * r1
        bound_a = 2.0 * float(gamma(n + m + k_max)) * float(np.dot(np.abs(v), np.concatenate([at, ab]) + np.abs(c1 * r1)))
        assert np.all(np.abs(y - y_np) <= 2.0 * gamma(k_max + 1) * (np.concatenate([at, ab]) + np.abs(c1 * r1)))
        assert abs(alfa - float(np.dot(v, y_np))) <= bound_a, (it, alfa, float(np.dot(v, y_np)), bound_a)
        assert np.array_equal(bits(ym), bits(mi * r2n) if with_minv else bits(r2n))
        s = float(np.dot(r2n, ym))
        bound_b = 2.0 * float(gamma(n + m + 1)) * float(np.dot(np.abs(r2n), np.abs(ym))) + 4.0 * 2.0 ** -53 * s
        assert abs(beta_new * beta_new - s) <= bound_b, (it, beta_new, s, bound_b)
        worst_a, worst_b = max(worst_a, abs(alfa - float(np.dot(v, y_np))) / bound_a), max(worst_b, abs(beta_new * beta_new - s) / bound_b)
    print("%s N=%d lifted=%s minv=%s diagonals=%s: %d iterations, alfa within %.4f and beta^2 within %.4f of their bounds"
          % (name, horizon, lifted, with_minv, diagonals, sol.iterations, worst_a, worst_b))
    return emu, pat, d, sol


@pytest.mark.parametrize("with_minv", [False, True])
@matrix([("periodic", 2), ("cost_ends", 3), ("stairs", 4), ("periodic", 30)])
def test_alfa_and_beta_of_every_iteration_against_numpy(model, name, horizon, lifted, with_minv):
    _, _, _, sol = alfa_and_beta_against_numpy(model, name, horizon, lifted, with_minv)
    assert sol.status == 0
    assert np.all(sol.trace[sol.iterations:, 5] == 0.0)     # the launches behind the last iteration found the trajectory frozen


# ---- 3b. omitted diagonals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diagonals", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("with_minv", [False, True])
@matrix([("periodic", 2), ("cost_ends", 3), ("stairs", 3), ("single", 4)])
def test_omitted_diagonals(model, name, horizon, lifted, with_minv, diagonals):
    """dx, dc or both left out (K.with_diagonals(None, None).solve): the apply launch then reads the bottom of v for the partial of v . y
    although the operator does not.  Without a diagonal these random K are singular (smallest singular value below 1e-17 in every layout
    tried: the random H has empty rows, and with m > n the (2, 2) block of zeros leaves J^T a null space), so there is no dense solve
    to compare with and no convergence; what is checked over 25 iterations instead: alfa and beta of every iteration against the numpy
    restatement with K of the SAME omitted diagonals (half of alfa lost would be far outside the bound), the estimate phibar / beta1
    equal to the true residual b - K z through the patterns, and a residual that never grows."""
    emu, pat, d, sol = alfa_and_beta_against_numpy(model, name, horizon, lifted, with_minv, diagonals=diagonals, maxiter=25)
    assert (sol.status, sol.iterations) == (1, 25) and (d["dx"] is None) == (not diagonals[0]) and (d["dc"] is None) == (not diagonals[1])
    true = true_residual(emu, pat, d, sol, with_minv)
    print("    residual %.6e, true %.6e" % (sol.residual, true))
    assert abs(sol.residual - true) <= 1e-8 and 0.0 < sol.residual < 1.0
    phibar = sol.trace[:, 2]
    assert np.all(phibar[1:] <= phibar[:-1])
    full = solve(model, name, horizon, lifted, False, 1e-8, with_minv, maxiter=25)[3]
    assert not np.array_equal(bits(full.top), bits(sol.top))           # (the diagonals do change the solve)


# ---- 4. - 7. freezing, the limit, b = 0, breakdown ---------------------------------------------------------------------------------------------
def same_bits(a, b):
    return (np.array_equal(bits(a.top), bits(b.top)) and np.array_equal(bits(a.bottom), bits(b.bottom)) and (a.iterations, a.status) == (b.iterations, b.status)
            and bits([a.residual])[0] == bits([b.residual])[0])


@pytest.mark.parametrize("with_minv", [False, True])
@matrix(CASES)
def test_a_converged_trajectory_is_frozen(model, name, horizon, lifted, with_minv):
    emu, pat, d, a = solve(model, name, horizon, lifted, False, 1e-8, with_minv, maxiter=300 if with_minv else 100)
    _, _, _, b = solve(model, name, horizon, lifted, False, 1e-8, with_minv, maxiter=340 if with_minv else 140)
    assert a.status == 0 and a.iterations < (300 if with_minv else 100)
    assert same_bits(a, b)
    assert np.array_equal(a.top_writes, b.top_writes) and np.array_equal(a.scalar_writes, b.scalar_writes)   # not a store more


@matrix(CASES)
def test_iteration_limit(model, name, horizon, lifted):
    emu, pat, d, sol = solve(model, name, horizon, lifted, False, 1e-8, False, maxiter=5)
    assert (sol.status, sol.iterations) == (1, 5) and 1e-8 < sol.residual < 1.0
    assert abs(sol.residual - true_residual(emu, pat, d, sol, False)) <= 1e-8
    _, _, _, zero = solve(model, name, horizon, lifted, False, 1e-8, False, maxiter=0)
    assert (zero.status, zero.iterations, zero.residual) == (1, 0, 1.0) and not zero.top.any() and not zero.bottom.any()


@pytest.mark.parametrize("with_minv", [False, True])
@matrix(CASES)
def test_a_zero_right_hand_side(model, name, horizon, lifted, with_minv):
    emu, _ = emu_of(model, name, horizon, lifted)
    d = inputs(emu, 7)
    sol = emu.solve(d["hess"], d["jac"], np.zeros(emu.n), np.zeros(emu.m), dx=d["dx"], dc=d["dc"], minv=(d["mt"], d["mb"]) if with_minv else None, maxiter=20)
    assert (sol.status, sol.iterations, sol.residual) == (0, 0, 0.0)
    assert np.array_equal(bits(sol.top), bits(np.zeros(emu.n))) and np.array_equal(bits(sol.bottom), bits(np.zeros(emu.m)))
    assert np.all(sol.top_writes == 1) and np.all(sol.bottom_writes == 1) and np.all(sol.scalar_writes == 1)


@matrix(CASES)
def test_a_preconditioner_that_is_not_positive_definite_is_a_breakdown(model, name, horizon, lifted):
    emu, _ = emu_of(model, name, horizon, lifted)
    d = inputs(emu, 8)
    mt, mb = np.ones(emu.n), np.ones(emu.m)
    j = int(np.argmax(np.abs(d["bt"])))
    mt[j] = -2.0 * (np.dot(d["bt"], d["bt"]) + np.dot(d["bb"], d["bb"]) - d["bt"][j] ** 2) / d["bt"][j] ** 2      # b . M^-1 b = -(the other squares)
    sol = emu.solve(d["hess"], d["jac"], d["bt"], d["bb"], dx=d["dx"], dc=d["dc"], minv=(mt, mb), maxiter=20)
    assert (sol.status, sol.iterations, sol.residual) == (2, 0, 1.0) and not sol.top.any() and not sol.bottom.any()
    bad = d["bt"].copy()
    bad[3] = np.inf                                                                                                 # and data that is not finite
    sol = emu.solve(d["hess"], d["jac"], bad, d["bb"], dx=d["dx"], dc=d["dc"], maxiter=20)
    assert (sol.status, sol.iterations) == (2, 0) and not sol.top.any() and not sol.bottom.any()
    hess = d["hess"].copy()
    hess[0] = np.nan                                                                                                # ... in the operator: the first alfa
    sol = emu.solve(hess, d["jac"], d["bt"], d["bb"], dx=d["dx"], dc=d["dc"], maxiter=20)
    assert (sol.status, sol.iterations) == (2, 0) and not sol.top.any() and not sol.bottom.any()                    # the last finite z


# ---- 8. the stores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_minv", [False, True])
@matrix(CASES)
def test_every_output_word_is_written(model, name, horizon, lifted, with_minv):
    """the destinations start as NaN (-99 for the integers); every element of the solution is stored once by the start and once per
    iteration taken, the three scalars likewise, and a frozen trajectory not once more"""
    for maxiter in (None, 5):
        emu, _, _, sol = solve(model, name, horizon, lifted, False, 1e-8, with_minv, maxiter=maxiter)
        assert sol.top_writes.shape == (emu.n,) and sol.bottom_writes.shape == (emu.m,)
        assert np.all(sol.top_writes == 1 + sol.iterations), np.flatnonzero(sol.top_writes != 1 + sol.iterations)[:8]
        assert np.all(sol.bottom_writes == 1 + sol.iterations), np.flatnonzero(sol.bottom_writes != 1 + sol.iterations)[:8]
        assert np.all(sol.scalar_writes == 1 + sol.iterations)
        assert np.all(np.isfinite(sol.top)) and np.all(np.isfinite(sol.bottom)) and np.isfinite(sol.residual) and sol.status in (0, 1) and sol.iterations >= 0
