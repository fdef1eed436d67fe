"""The KKT chain of the pose finder from stored value runs (hippopt_amd/csrc/pose_kkt.h: the operator, the diagonal preconditioner and the
whole MINRES solve of one pose in one workgroup), run by the CPU emulation of the three kernels (tests/pose_kkt_emu) for all six settings
variants: the tables, K e_j against the dense matrix bit for bit, random products within their rounding bound, the diagonal within the
bounds of tests/test_kkt_precond_hostemu.py, the stores, and the solve — on the synthetic inputs of pose_kkt_check.inputs (0.05 N(0,1) and
0.02 N(0,1) value runs, dx, dc in U[1, 2]; identity, a random diagonal, the built diagonal), on their symmetric rescaling S K S at
cond about 1e12, and on the REAL value runs of the three poses of pose_products_check.workload(name, st, model, 2100).

Measured with this emulation (rtol 1e-8; printed by the tests): synthetic identity 34 to 38 iterations, random diagonal 75 to 91, built
diagonal 17 (0.05) and 11 (0.02), the counts of the numpy restatement but one (80 for 79); rescaled (cond 3.9e11 to 1.4e12) with the built
diagonal exactly the unscaled counts; the 18 real systems with the built diagonal 75 to 349 iterations, all status 0 (the counts per
system: DESIGN.md).  CPU only."""
import numpy as np
import pytest

import pose_kkt_check as pkc
import pose_products_check as ppc
from hvp_check import gamma, touch_counts
from kkt_check import apply, bits
from test_kkt_precond_hostemu import assert_against_numpy
from test_pose_body_hostemu import VARIANTS, variants

RTOL = 1e-8
_EMU, _REAL = {}, {}


def emu_of(model, name):
    """(emulation, patterns (hr, hc, ir, jc), synthetic inputs, real inputs) of a variant, made once"""
    from pose_kkt_emu_lib import PoseKktEmu
    if name not in _EMU:
        e = PoseKktEmu(variants(model)[name], model)
        ir, jc, hr, hc = e.sparsity()
        _EMU[name] = (e, (hr, hc, ir, jc)) + pkc.inputs(e.n, e.m, e.nnz, e.hnnz)
    return _EMU[name]


def real_runs(model, name):
    """the real systems of a variant: for each of the three poses a dict hess, jac, dx, dc, bt, bb — the value runs from the emulation
    of the pose kernels (tests/pose_products_emu), computed once"""
    from pose_products_emu_lib import PoseProductsEmu
    if name not in _REAL:
        e, _, _, real = emu_of(model, name)
        st = variants(model)[name]
        pe = PoseProductsEmu(st, model)
        x, p = ppc.workload(name, st, model, pkc.WORKLOAD_SEED)
        lam, sigma, _ = ppc.factors(e.m, e.n, pkc.FACTOR_SEED)
        _REAL[name] = [dict(real[b], jac=pe.eval(x[b], p[b])[3], hess=pe.hess(x[b], p[b], sigma[b], lam[b])) for b in range(3)]
    return _REAL[name]


def once(*buffers):
    return all(np.all(w == 1) for w in buffers)


# ---- 1. tables --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_tables(model, name):
    e, (hr, hc, ir, jc), _, _ = emu_of(model, name)
    dev, own = e.device_words(), e.device_words(own=True)
    for key in dev:
        assert np.array_equal(dev[key], own[key]), key                  # PoseLayout::fill_kkt_tables against the emulation's own statement
    assert np.array_equal(dev["col_word"][:e.nnz] & 4095, np.arange(e.nnz)) and np.array_equal(dev["col_word"][:e.nnz] >> 12, ir)
    ent = dev["row_word"][:e.nnz] & 4095
    assert np.array_equal(np.sort(ent), np.arange(e.nnz)) and np.array_equal(dev["row_word"][:e.nnz] >> 12, jc[ent])
    assert np.all(np.diff(ir[ent]) >= 0)                                 # row after row ...
    assert np.all((np.diff(jc[ent]) > 0) | (np.diff(ir[ent]) > 0))       # ... each in ascending column
    ntouch = int(touch_counts(hr, hc, e.n).sum())
    pos, other = dev["touch_word"][:ntouch] & 4095, dev["touch_word"][:ntouch] >> 12
    assert np.all(((hr[pos] == other) | (hc[pos] == other)) & (pos < e.hnnz))
    assert not dev["col_word"][e.nnz:].any() and not dev["row_word"][e.nnz:].any() and not dev["touch_word"][ntouch:].any()
    hd = e.hdiag()
    assert np.array_equal(dev["hdiag"][:e.n], hd) and np.all(dev["hdiag"][e.n:] == -1)
    for c in range(e.n):
        on = np.flatnonzero((hr == c) & (hc == c))
        assert hd[c] == (on[0] if on.size else -1), c
    none = int(np.count_nonzero(hd < 0))
    print("%s: n %d m %d nnz %d hnnz %d touches %d, %d variables without a diagonal Hessian entry" % (name, e.n, e.m, e.nnz, e.hnnz, ntouch, none))
    assert (none == 0) if name.startswith("hands") else (3 <= none <= 15)
    assert e.nnz <= e.ent_cap and e.m <= e.row_cap and ntouch <= e.touch_cap and e.hnnz <= e.hess_cap and e.n <= 128


# ---- 2. the operator --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diagonals", [(True, True), (False, False)])
@pytest.mark.parametrize("name", VARIANTS)
def test_unit_vectors_return_the_columns_of_the_dense_matrix(model, name, diagonals):
    e, pat, syn, _ = emu_of(model, name)
    d = syn[0]
    dx, dc = (d["dx"] if diagonals[0] else None), (d["dc"] if diagonals[1] else None)
    K = pkc.dense(e.n, e.m, pat, d["hess"], d["jac"], dx, dc)
    for j in range(e.n + e.m):
        unit = np.zeros(e.n + e.m)
        unit[j] = 1.0
        got = e.times(d["hess"], d["jac"], unit[:e.n], unit[e.n:], dx, dc)
        assert np.array_equal(np.concatenate([got.top, got.bottom]), K[:, j]), j      # (also the variables without a Hessian diagonal)
        assert once(got.top_writes, got.bottom_writes)


@pytest.mark.parametrize("diagonals", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("name", VARIANTS)
def test_random_products_within_the_rounding_bound(model, name, diagonals):
    e, pat, syn, _ = emu_of(model, name)
    hr, hc, ir, jc = pat
    rng = np.random.RandomState(5)
    k_top = touch_counts(hr, hc, e.n) + np.bincount(jc, minlength=e.n) + 1
    k_bot = np.bincount(ir, minlength=e.m) + 1
    for d in syn + real_runs(model, name)[:1]:
        dx, dc = (d["dx"] if diagonals[0] else None), (d["dc"] if diagonals[1] else None)
        v, w = rng.standard_normal(e.n), rng.standard_normal(e.m)
        got = e.times(d["hess"], d["jac"], v, w, dx, dc)
        rt, rb = apply(e.n, e.m, hr, hc, d["hess"], ir, jc, d["jac"], dx, dc, v, w)
        at, ab = apply(e.n, e.m, hr, hc, d["hess"], ir, jc, d["jac"], dx, dc, v, w, absolute=True)
        assert np.all(np.abs(got.top - rt) <= 2.0 * gamma(k_top + 1) * at) and np.all(np.abs(got.bottom - rb) <= 2.0 * gamma(k_bot + 1) * ab)
        assert once(got.top_writes, got.bottom_writes)


# ---- 3. the diagonal --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diagonals", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("name", VARIANTS)
def test_diagonal_against_numpy(model, name, diagonals):
    e, pat, syn, _ = emu_of(model, name)
    for what, d in (("synthetic 0.05", syn[0]), ("real pose 0", real_runs(model, name)[0])):
        dx, dc = (d["dx"] if diagonals[0] else None), (d["dc"] if diagonals[1] else None)
        got = e.diagonal_preconditioner(d["hess"], d["jac"], dx, dc, 1e-10)
        assert_against_numpy(e, pat, d["hess"], d["jac"], dx, dc, got, "%s %s diagonals=%s" % (name, what, diagonals))
        assert once(got.top_writes, got.bottom_writes)
    if not diagonals[0]:                                                  # a variable without a Hessian entry and without dx: the floor
        none = np.flatnonzero(e.hdiag() < 0)
        assert np.all(got.top[none] == 1e10)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_value_that_is_not_finite_comes_out_as_nan(model, bad):
    e, pat, syn, _ = emu_of(model, "default")
    hr, hc, ir, jc = pat
    d = syn[0]
    clean = e.diagonal_preconditioner(d["hess"], d["jac"], d["dx"], d["dc"])
    jac = d["jac"].copy()
    jac[e.nnz // 2] = bad
    got = e.diagonal_preconditioner(d["hess"], jac, d["dx"], d["dc"])
    row = ir[e.nnz // 2]
    assert np.isnan(got.bottom[row]) and np.array_equal(bits(np.delete(got.bottom, row)), bits(np.delete(clean.bottom, row))) and np.array_equal(bits(got.top), bits(clean.top))
    dx = d["dx"].copy()
    dx[7] = bad
    got = e.diagonal_preconditioner(d["hess"], d["jac"], dx, d["dc"])
    rows = np.unique(ir[jc == 7])
    assert np.isnan(got.top[7]) and np.all(np.isnan(got.bottom[rows])) and np.array_equal(bits(np.delete(got.top, 7)), bits(np.delete(clean.top, 7)))


# ---- 4. the solve on synthetic inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_synthetic_systems_converge(model, name):
    e, pat, syn, _ = emu_of(model, name)
    for scale, d in zip(pkc.SCALES, syn):
        K = pkc.dense(e.n, e.m, pat, d["hess"], d["jac"], d["dx"], d["dc"])
        b = np.concatenate([d["bt"], d["bb"]])
        for what, minv in (("identity", None), ("random", (d["mt"], d["mb"])), ("built", "diagonal")):
            sol = e.solve(d["hess"], d["jac"], d["bt"], d["bb"], d["dx"], d["dc"], minv=minv, rtol=RTOL, maxiter=100)
            true = pkc.residual_2norm(e.n, e.m, pat, d, sol.top, sol.bottom)
            mv = np.ones(e.n + e.m) if minv is None else np.concatenate(minv if what == "random" else pkc.numpy_diagonal(e.n, e.m, pat, d["hess"], d["jac"], d["dx"], d["dc"]))
            its = pkc.numpy_minres(K, b, mv, RTOL, 100)[0]
            print("%s synthetic %.2f %s: status %d after %d iterations (numpy: %d), residual %.3e, 2-norm residual %.3e" % (name, scale, what, sol.status, sol.iterations, its, sol.residual, true))
            assert sol.status == 0 and 0 < sol.iterations <= 100 and sol.residual <= RTOL
            assert once(sol.top_writes, sol.bottom_writes, sol.scalar_writes)
            if minv is None:
                assert true <= 10.0 * RTOL                               # (a wrong operator or recurrence leaves O(1))


@pytest.mark.parametrize("name", VARIANTS)
def test_rescaled_systems_converge_with_the_built_diagonal_in_the_unscaled_count(model, name):
    e, pat, syn, _ = emu_of(model, name)
    for scale, d in zip(pkc.SCALES, syn):
        r = pkc.rescaled(d, pat)
        cond = float(np.linalg.cond(pkc.dense(e.n, e.m, pat, r["hess"], r["jac"], r["dx"], r["dc"])))
        base = e.solve(d["hess"], d["jac"], d["bt"], d["bb"], d["dx"], d["dc"], minv="diagonal", rtol=RTOL, maxiter=100)
        sol = e.solve(r["hess"], r["jac"], r["bt"], r["bb"], r["dx"], r["dc"], minv="diagonal", floor=1e-300, rtol=RTOL, maxiter=100)
        print("%s synthetic %.2f rescaled: cond %.2e, status %d after %d iterations (unscaled: %d)" % (name, scale, cond, sol.status, sol.iterations, base.iterations))
        assert cond > 1e10
        assert base.status == 0 and sol.status == 0 and abs(sol.iterations - base.iterations) <= 2


# ---- 5. real value runs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_real_value_runs_converge_with_the_built_diagonal(model, name):
    """all 18 (variant, pose) systems, none left out: status 0 within 1 000 iterations"""
    e, pat, _, _ = emu_of(model, name)
    for b, d in enumerate(real_runs(model, name)):
        sol = e.solve(d["hess"], d["jac"], d["bt"], d["bb"], d["dx"], d["dc"], minv="diagonal", rtol=RTOL, maxiter=1000)
        true = pkc.residual_2norm(e.n, e.m, pat, d, sol.top, sol.bottom)
        print("%s real pose %d: |H| up to %.1e, status %d after %d iterations, residual %.3e, 2-norm residual %.3e" % (name, b, np.abs(d["hess"]).max(), sol.status, sol.iterations, sol.residual, true))
        assert sol.status == 0 and 0 < sol.iterations <= 1000 and sol.residual <= RTOL
        assert once(sol.top_writes, sol.bottom_writes, sol.scalar_writes)


# ---- 6. statuses ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minv", [None, "given", "diagonal"])
@pytest.mark.parametrize("name", VARIANTS)
def test_a_zero_right_hand_side(model, name, minv):
    e, _, syn, _ = emu_of(model, name)
    d = syn[0]
    sol = e.solve(d["hess"], d["jac"], np.zeros(e.n), np.zeros(e.m), d["dx"], d["dc"], minv=(d["mt"], d["mb"]) if minv == "given" else minv, maxiter=20)
    assert (sol.status, sol.iterations, sol.residual) == (0, 0, 0.0)
    assert np.array_equal(bits(sol.top), bits(np.zeros(e.n))) and np.array_equal(bits(sol.bottom), bits(np.zeros(e.m)))
    assert once(sol.top_writes, sol.bottom_writes, sol.scalar_writes)


@pytest.mark.parametrize("name", VARIANTS)
def test_iteration_limit(model, name):
    e, pat, syn, _ = emu_of(model, name)
    d = syn[0]
    sol = e.solve(d["hess"], d["jac"], d["bt"], d["bb"], d["dx"], d["dc"], maxiter=5)
    assert (sol.status, sol.iterations) == (1, 5) and RTOL < sol.residual < 1.0
    assert abs(sol.residual - pkc.residual_2norm(e.n, e.m, pat, d, sol.top, sol.bottom)) <= 1e-8       # (identity: the M^-1 norm is the 2-norm)
    zero = e.solve(d["hess"], d["jac"], d["bt"], d["bb"], d["dx"], d["dc"], maxiter=0)
    assert (zero.status, zero.iterations, zero.residual) == (1, 0, 1.0) and not zero.top.any() and not zero.bottom.any()
    assert once(sol.top_writes, sol.bottom_writes, sol.scalar_writes, zero.top_writes, zero.bottom_writes, zero.scalar_writes)


@pytest.mark.parametrize("name", VARIANTS)
def test_breakdown_leaves_the_solution_as_it_was(model, name):
    e, _, syn, _ = emu_of(model, name)
    d = syn[0]
    mt, mb = np.ones(e.n), np.ones(e.m)
    j = int(np.argmax(np.abs(d["bt"])))
    mt[j] = -2.0 * (np.dot(d["bt"], d["bt"]) + np.dot(d["bb"], d["bb"]) - d["bt"][j] ** 2) / d["bt"][j] ** 2      # b . M^-1 b = -(the other squares)
    sol = e.solve(d["hess"], d["jac"], d["bt"], d["bb"], d["dx"], d["dc"], minv=(mt, mb), maxiter=20)
    assert (sol.status, sol.iterations, sol.residual) == (2, 0, 1.0) and not sol.top.any() and not sol.bottom.any()
    for run in ("hess", "jac"):                                                                                     # a NaN in a value run: the first alfa
        bad = dict(d)
        bad[run] = d[run].copy()
        bad[run][3] = np.nan
        for minv in (None, "diagonal"):
            sol = e.solve(bad["hess"], bad["jac"], d["bt"], d["bb"], d["dx"], d["dc"], minv=minv, maxiter=20)
            assert (sol.status, sol.iterations) == (2, 0) and not sol.top.any() and not sol.bottom.any(), (run, minv)
            assert once(sol.top_writes, sol.bottom_writes, sol.scalar_writes)


# ---- 7. the diagonal built inside the solve -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_build_diagonal_is_the_preconditioner_call_then_minv(model, name):
    e, _, syn, _ = emu_of(model, name)
    for d, diagonals in ((syn[1], (True, True)), (real_runs(model, name)[1], (True, True)), (syn[0], (False, True)), (syn[0], (True, False))):
        dx, dc = (d["dx"] if diagonals[0] else None), (d["dc"] if diagonals[1] else None)
        m = e.diagonal_preconditioner(d["hess"], d["jac"], dx, dc, 1e-9)
        a = e.solve(d["hess"], d["jac"], d["bt"], d["bb"], dx, dc, minv=(m.top, m.bottom), maxiter=60)
        b = e.solve(d["hess"], d["jac"], d["bt"], d["bb"], dx, dc, minv="diagonal", floor=1e-9, maxiter=60)
        assert a.iterations > 5 and (a.iterations, a.status) == (b.iterations, b.status) and bits([a.residual])[0] == bits([b.residual])[0]
        assert np.array_equal(bits(a.top), bits(b.top)) and np.array_equal(bits(a.bottom), bits(b.bottom))
