"""The Hessian-vector product y = H(x, sigma, lambda) v of the knot-local reduction (hippopt_amd/csrc/knot_hvp.h over the touch tables
HessLayout::build records), run by the CPU emulation of hipnlp_knot_hvp_kernel and hipnlp_hess_times_kernel (tests/hvp_emu): against the
oracle and the reference planner's fixtures with the bounds of tests/hvp_check.py, every output written exactly once, the fused and the
stored-values variant bitwise the same.  CPU only."""
import json
import os

import numpy as np
import pytest

from hvp_check import check, full_multipliers, gamma, oracle_bound, own_bound, rel, sym_times, touch_counts
from test_lagrangian_grad_hostemu import MAKERS, SMOOTH, sigmas, workload

NXK = 189
CASES = [("periodic", 2), ("periodic", 3), ("periodic", 7), ("single", 7), ("cost_ends", 7), ("stairs", 3), ("stairs", 6), ("ramp", 6)]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("name,horizon", CASES)
def test_emulated_hessian_vector_product_matches_oracle(model, name, horizon, lifted):
    from hvp_emu_lib import HvpEmu
    from oracle_lib import Oracle
    seed = 500 + horizon + 17 * list(MAKERS).index(name)
    st, x, p = workload(name, model, horizon, seed)
    emu = HvpEmu(st, model, detect_simple_bounds=lifted)
    orc = Oracle(st, model)
    ir, jc = emu.hess_sparsity()
    k_i = emu.touch_counts()
    assert np.array_equal(k_i, touch_counts(ir, jc, emu.n))
    rng = np.random.RandomState(seed)
    lam = rng.standard_normal(emu.m)
    lam_full = full_multipliers(lam, emu.kept_rows())
    vs = [rng.standard_normal(emu.n) for _ in range(3)]
    for sigma in sigmas(seed):
        iro, jco, valo = orc.hess(x, p, sigma, lam_full)
        for j, v in enumerate(vs):
            y, _ = emu.hess_vec(x, p, sigma, lam, v)
            ref, bound = oracle_bound(iro, jco, valo, ir, jc, v, k_i, name in SMOOTH)
            check(y, ref, bound, "%s N=%d lifted=%s sigma=%g v%d" % (name, horizon, lifted, sigma, j))


@pytest.mark.parametrize("name", ["planner_periodic_N3", "planner_single_N3", "planner_costends_N2", "planner_stairs_N3", "planner_ramp_N3"])
def test_emulated_product_matches_reference_planner_fixture(model, name):
    from hvp_emu_lib import HvpEmu
    from test_golden_planner import GOLD, settings_for
    z = np.load(os.path.join(GOLD, name + ".npz"))
    emu = HvpEmu(settings_for(json.loads(str(z["meta"])), model), model)
    dirs, want = np.asarray(z["hess_dirs"]), np.asarray(z["hess_times_dirs"])
    dirs, want = (dirs, want) if dirs.shape[-1] == emu.n else (dirs.T, want.T)
    assert dirs.shape == (4, emu.n)
    for j in range(4):
        y, _ = emu.hess_vec(z["x"], z["p"], float(z["hess_sigma"]), z["hess_lambda"], dirs[j])
        e = rel(y, want[j])
        print("%s direction %d: rel %.3e" % (name, j, e))
        assert e < (1e-9 if ("stairs" in name or "ramp" in name) else 1e-11)


@pytest.mark.parametrize("horizon", [2, 6])
@pytest.mark.parametrize("name", ["periodic", "cost_ends", "stairs"])
def test_every_output_is_written_exactly_once(model, name, horizon):
    from hvp_emu_lib import HvpEmu
    st, x, p = workload(name, model, horizon, 9)
    emu = HvpEmu(st, model)
    assert (emu.n_couple > 0) == (name == "cost_ends")
    rng = np.random.RandomState(2)
    lam, v = rng.standard_normal(emu.m), rng.standard_normal(emu.n)
    out = np.full(emu.n, np.nan)
    y, writes, values = emu.hess_vec(x, p, 1.3, lam, v, out=out, want_values=True)
    assert y is out
    assert np.array_equal(writes, np.ones(emu.n, np.int32)), np.flatnonzero(writes != 1)
    assert np.all(np.isfinite(out))
    assert np.array_equal(bits(out[NXK * horizon:]), np.zeros(6, np.int64))   # the six horizon-global entries: exactly +0.0
    out2 = np.full(emu.n, np.nan)
    _, writes2 = emu.hess_times(values, v, out=out2)
    assert np.array_equal(writes2, np.ones(emu.n, np.int32))
    assert np.array_equal(bits(out2[NXK * horizon:]), np.zeros(6, np.int64))


@pytest.mark.parametrize("name", list(MAKERS))
def test_touch_tables_are_the_pattern_row_by_row_and_column_by_column(model, name):
    from hvp_emu_lib import HvpEmu
    N = 4
    emu = HvpEmu(MAKERS[name](N, model), model)
    t = emu.tables()
    ir, jc = emu.hess_sparsity()
    perm, _ = emu.perm()
    nk = emu.nnz_knot
    assert nk == (1878 if name in SMOOTH else 1539) and emu.nnz_h == nk * N + emu.n_couple
    assert emu.n_couple == (84 if name == "cost_ends" else 0)
    assert ir.max() < NXK * N                                              # no entry touches the horizon-global variables
    lr, lc = ir[:nk], jc[:nk]                                              # knot 0's block: offsets inside the record
    for k in range(N):
        assert np.array_equal(ir[nk * k:nk * (k + 1)] - NXK * k, lr) and np.array_equal(jc[nk * k:nk * (k + 1)] - NXK * k, lc)
    assert emu.touches == (3567 if name in SMOOTH else 2889) == int(t["beg"][-1]) and emu.touches <= 14 * 256
    assert np.array_equal(np.diff(t["beg"]), t["K"]) and t["K"].max() == 54 and t["K"].min() >= 1
    for i in range(NXK):
        e = slice(t["beg"][i], t["beg"][i + 1])
        want = np.flatnonzero((lr == i) | (lc == i))                       # block-position order
        assert np.array_equal(t["pos"][e], want), i
        assert np.array_equal(t["other"][e], np.where(lr[want] == i, lc[want], lr[want])), i
        assert np.array_equal(t["slot"][e], perm[want]), i
    assert np.any((lr == lc) & True) and np.all(np.isin(np.arange(NXK), lr[lr == lc]))   # every variable has a diagonal entry
    seen = np.bincount(t["pos"], minlength=nk)
    assert np.array_equal(seen, np.where(lr == lc, 1, 2))                  # every position once (diagonal) or twice
    cr, cc = ir[nk * N:] - NXK * (N - 1), jc[nk * N:]
    assert np.array_equal(cr, cc)                                          # the coupling pairs a variable with itself
    want_couple = np.full(NXK, -1)
    want_couple[cr] = np.arange(emu.n_couple)
    assert np.array_equal(t["couple"], want_couple)
    assert np.array_equal(emu.touch_counts(), touch_counts(ir, jc, emu.n))


@pytest.mark.parametrize("name,horizon", [("periodic", 5), ("cost_ends", 2), ("cost_ends", 5), ("stairs", 4), ("ramp", 3)])
def test_fused_and_stored_values_agree_bitwise_and_the_product_is_symmetric(model, name, horizon):
    from hostemu_lib import HostEmu
    from hvp_emu_lib import HvpEmu
    st, x, p = workload(name, model, horizon, 77)
    emu = HvpEmu(st, model)
    rng = np.random.RandomState(8)
    lam, v, w = rng.standard_normal(emu.m), rng.standard_normal(emu.n), rng.standard_normal(emu.n)
    yv, _, values = emu.hess_vec(x, p, 0.6, lam, v, want_values=True)
    assert np.array_equal(bits(values), bits(HostEmu(st, model).hess(x, p, 0.6, lam)))   # the value run is the existing emulation's
    ys, _ = emu.hess_times(values, v)
    assert np.array_equal(bits(yv), bits(ys))
    yw, _ = emu.hess_times(values, w)
    assert np.array_equal(bits(yw), bits(emu.hess_vec(x, p, 0.6, lam, w)[0]))
    # own-values bound, and  w . (H v) == v . (H w)  within the bounds of the two sums (each y_i carries gamma_{K_i} S_i, the dot n more)
    ir, jc = emu.hess_sparsity()
    k_i = emu.touch_counts()
    ref, bound = own_bound(ir, jc, values, v, k_i)
    check(yv, ref, bound, "%s N=%d own values" % (name, horizon))
    a, b = float(np.dot(w, yv)), float(np.dot(v, yw))
    slack = (gamma(k_i.max() + emu.n) * (np.dot(np.abs(w), sym_times(ir, jc, values, v, absolute=True)) + np.dot(np.abs(v), sym_times(ir, jc, values, w, absolute=True))))
    print("%s N=%d: w.Hv - v.Hw = %.3e (bound %.3e)" % (name, horizon, a - b, slack))
    assert abs(a - b) <= slack


@pytest.mark.parametrize("name", ["periodic", "cost_ends", "stairs"])
def test_zero_sigma_and_zero_multipliers_give_exactly_zero(model, name):
    from hvp_emu_lib import HvpEmu
    st, x, p = workload(name, model, 4, 3)
    emu = HvpEmu(st, model)
    y, _ = emu.hess_vec(x, p, 0.0, np.zeros(emu.m), np.random.RandomState(1).standard_normal(emu.n))
    assert np.array_equal(y, np.zeros(emu.n))
