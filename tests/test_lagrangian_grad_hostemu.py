"""The Lagrangian gradient xbar = sigma grad f + J^T lambda of the knot-local reduction (hippopt_amd/csrc/knot_lgrad.h over the tables
Layout::build records), run by the CPU emulation of hipnlp_knot_lgrad_kernel (tests/lgrad_emu): against the oracle with the bound of
tests/lgrad_check.py, bitwise the same for both jac orders, every output written exactly once.  CPU only."""
import numpy as np
import pytest

from hippopt_amd import _abi
from hippopt_amd.kinodyn_settings import periodic_step_settings, ramp_settings, single_step_settings, stairs_settings
from hippopt_amd.synthetic import make_workload, place_on_step_flanks
from lgrad_check import TOL_PLANAR, TOL_SMOOTH, check, column_counts, full_multipliers, oracle_bound


def periodic_cost_ends_settings(horizon, model):
    """periodic step with the final state and the periodicity as costs (EXPR_MINIMIZE)"""
    st = periodic_step_settings(horizon, model)
    st.final_state_expression_type = _abi.EXPR_MINIMIZE
    st.final_state_expression_weight = 3.0
    st.periodicity_expression_type = _abi.EXPR_MINIMIZE
    st.periodicity_expression_weight = 0.7
    return st


MAKERS = {"periodic": periodic_step_settings, "single": single_step_settings, "cost_ends": periodic_cost_ends_settings,
          "stairs": stairs_settings, "ramp": ramp_settings}
SMOOTH = ("stairs", "ramp")


def workload(name, model, horizon, seed):
    st = MAKERS[name](horizon, model)
    x, p = make_workload(st, model, batch=1, seed=seed)
    if name in SMOOTH:
        place_on_step_flanks(x[0], st, seed=seed)
    return st, x[0], p[0]


def sigmas(seed):
    return (1.0, 0.0, float(np.random.RandomState(seed).uniform(0.1, 3.0)))


@pytest.mark.parametrize("vary_first", [False, True])
@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("name,horizon", [("periodic", 2), ("periodic", 3), ("periodic", 7), ("single", 7), ("cost_ends", 7), ("stairs", 3), ("stairs", 6), ("ramp", 6)])
def test_emulated_lagrangian_gradient_matches_oracle(model, name, horizon, lifted, vary_first):
    from lgrad_emu_lib import LgradEmu
    from oracle_lib import Oracle
    seed = 300 + horizon + 17 * list(MAKERS).index(name)
    st, x, p = workload(name, model, horizon, seed)
    emu = LgradEmu(st, model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
    ok, why = emu.tables_ok()
    assert ok, why
    orc = Oracle(st, model)
    _, grado, _, jaco = orc.eval(x, p)
    iro, jco = orc.sparsity()
    _, jc = emu.sparsity()
    k_c = column_counts(jc, emu.n)
    lam = np.random.RandomState(seed).standard_normal(emu.m)
    lam_full = full_multipliers(lam, emu.kept_rows())
    tol = TOL_SMOOTH if name in SMOOTH else TOL_PLANAR
    for sigma in sigmas(seed):
        xbar, _ = emu.lagrangian_grad(x, p, sigma, lam)
        ref, bound = oracle_bound(grado, iro, jco, jaco, sigma, lam_full, k_c, tol)
        check(xbar, ref, bound, "%s N=%d lifted=%s vary_first=%s sigma=%g" % (name, horizon, lifted, vary_first, sigma))


@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("name", ["periodic", "cost_ends", "stairs", "ramp"])
def test_ccs_and_varying_first_give_the_same_bits(model, name, lifted):
    from lgrad_emu_lib import LgradEmu
    st, x, p = workload(name, model, 5, 41)
    ccs = LgradEmu(st, model, detect_simple_bounds=lifted)
    vf = LgradEmu(st, model, detect_simple_bounds=lifted, jac_varying_first=True)
    ir_c, jc_c = ccs.sparsity()
    ir_v, jc_v = vf.sparsity()
    assert not (np.array_equal(ir_c, ir_v) and np.array_equal(jc_c, jc_v))   # (the two orders of a block really differ)
    lam = np.random.RandomState(5).standard_normal(ccs.m)
    a, _ = ccs.lagrangian_grad(x, p, 0.75, lam)
    b, _ = vf.lagrangian_grad(x, p, 0.75, lam)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("name,horizon", [("periodic", 2), ("periodic", 6), ("stairs", 6), ("single", 4)])
def test_every_output_is_written_exactly_once(model, name, horizon):
    from lgrad_emu_lib import LgradEmu
    st, x, p = workload(name, model, horizon, 9)
    for lifted in (False, True):
        emu = LgradEmu(st, model, detect_simple_bounds=lifted)
        out = np.full(emu.n, np.nan)
        xbar, writes = emu.lagrangian_grad(x, p, 1.3, np.random.RandomState(2).standard_normal(emu.m), out=out)
        assert xbar is out
        assert np.array_equal(writes, np.ones(emu.n, np.int32)), np.flatnonzero(writes != 1)
        assert np.all(np.isfinite(out))


def test_tables_cover_the_pattern_and_fit_the_kernel(model):
    """the recorded entries of the three variants and of the horizon-global columns are the pattern of jac g, column by column"""
    from lgrad_emu_lib import LgradEmu
    for name in MAKERS:
        for lifted in (False, True):
            st = MAKERS[name](4, model)
            emu = LgradEmu(st, model, detect_simple_bounds=lifted)
            ok, why = emu.tables_ok()
            assert ok, (name, lifted, why)
            entries, rows, glob = emu.table_sizes()
            _, jc = emu.sparsity()
            n_knot = [int(((jc // 189) == k).sum()) for k in range(4)]
            assert entries == [n_knot[0], n_knot[1], n_knot[3]] and n_knot[2] == n_knot[1], (name, lifted)
            assert glob == int((jc >= 189 * 4).sum())
            assert max(rows) <= 2 * 256 and max(entries) <= 7 * 256
