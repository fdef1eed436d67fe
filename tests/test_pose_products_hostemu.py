"""The pose finder's workgroup-local products (hippopt_amd/csrc/pose_products.h) and the directories of PoseLayout::build_product_tables
through the TEST-ONLY CPU emulation of the three kernels (tests/pose_products_emu), against the emulation's own outputs, the AD oracle and
the golden vectors of the reference's pose finder.  The same accuracy checks on the GPU: test_gpu_pose_products.py."""
import json
import os

import numpy as np
import pytest

import pose_products_check as ppc
from oracle_lib import PoseOracle
from pose_products_emu_lib import PoseProductsEmu, set_wave_order
from test_golden_pose import GOLD, pose_settings_for
from test_pose_body_hostemu import VARIANTS, variants


@pytest.fixture(scope="module")
def emus(model):
    """one emulation handle per settings variant (the layout is recorded once)"""
    st = variants(model)
    return {name: (st[name], PoseProductsEmu(st[name], model)) for name in VARIANTS}


def all_products(e, x, p, sigma, lam, v):
    """(xbar, grad f . v, J v, H v) of one pose, every store counted and every guard word checked"""
    xb = e.lagrangian_grad(x, p, sigma, lam)
    d, jv = e.jac_vec(x, p, v)
    hv = e.hess_vec(x, p, sigma, lam, v)
    for b in (xb, d, jv, hv):
        assert np.all(b.writes == 1), b.writes
        assert b.intact()
    return xb.out.copy(), float(d.out[0]), jv.out.copy(), hv.out.copy()


@pytest.mark.parametrize("name", VARIANTS)
def test_products_match_own_outputs_and_oracle(model, emus, name):
    st, e = emus[name]
    o = PoseOracle(st, model)
    ir, jc, hr, hc = e.sparsity()
    iro, jco = o.sparsity()
    assert np.array_equal(ir, iro) and np.array_equal(jc, jco)
    x, p = ppc.workload(name, st, model, 2100)
    lam, sigma, v = ppc.factors(e.m, e.n, 31)
    for b in range(3):
        xbar, dot, jv, hv = all_products(e, x[b], p[b], sigma[b], lam[b], v[b])
        _, grad, _, jac = e.eval(x[b], p[b])
        _, grado, _, jaco = o.eval(x[b], p[b])
        ppc.check_first_order("%s pose %d" % (name, b), (ir, jc), (grad, jac), (grado, jaco), (xbar, dot, jv), float(sigma[b]), lam[b], v[b])
        vals = e.hess(x[b], p[b], sigma[b], lam[b])
        Href = o.hess(x[b], p[b], float(sigma[b]), lam[b])
        ppc.check_second_order("%s pose %d" % (name, b), (hr, hc), vals, Href, hv, v[b], ppc.tol_h(name))
    assert e.map_violations() == 0   # (the pose program ran on the device emitter's cut staging: every emission was one the device can serve)


@pytest.mark.parametrize("name", ["pose_default", "pose_step_constrained", "pose_hands"])
def test_products_match_reference_fixture(model, name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    st = pose_settings_for(json.loads(str(z["meta"])), model)
    e = PoseProductsEmu(st, model)
    ir, jc, hr, hc = e.sparsity()
    rng = np.random.RandomState(17)
    v = rng.standard_normal(e.n)
    sigma, lam = float(z["hess_sigma"]), np.asarray(z["hess_lambda"], dtype=np.float64)
    xbar, dot, jv, hv = all_products(e, z["x"], z["p"], sigma, lam, v)
    # H v against the fixture's dense Hessian at the fixture's sigma and lambda
    k_i = ppc.hvp_check.touch_counts(hr, hc, e.n)
    ref, bound = ppc.dense_hess_bound(z["hess"], hr, hc, v, k_i, 1e-10)
    ppc.hvp_check.check(hv, ref, bound, name + ": H v against the fixture")
    # xbar and J v against the fixture's grad and triplets (entries outside the pattern are zeros there: test_pose_body_matches_reference_fixture)
    fr, fc, fv = np.asarray(z["jac_row"], dtype=np.int64), np.asarray(z["jac_col"], dtype=np.int64), np.asarray(z["jac_val"], dtype=np.float64)
    pos = {(int(r), int(c)): i for i, (r, c) in enumerate(zip(ir, jc))}
    jref = np.zeros(e.nnz)
    for r, c, val in zip(fr, fc, fv):
        i = pos.get((int(r), int(c)))
        if i is None:
            assert abs(val) < 1e-12, ("entry outside the pattern", r, c, val)
        else:
            jref[i] = val
    grad = np.asarray(z["grad"], dtype=np.float64)
    k_c = ppc.lgrad_check.column_counts(jc, e.n)
    ref, bound = ppc.lgrad_check.oracle_bound(grad, ir, jc, jref, sigma, lam, k_c, 1e-10)
    ppc.lgrad_check.check(xbar, ref, bound, name + ": xbar against the fixture")
    k_r = np.bincount(ir, minlength=e.m)
    ref = ppc.row_times(ir, jc, jref, v, e.m)
    bound = 1e-10 * ppc.row_times(ir, jc, jref, v, e.m, floor=True) + 2.0 * ppc.lgrad_check.gamma(k_r + 1) * ppc.row_times(ir, jc, jref, v, e.m, absolute=True)
    ppc.lgrad_check.check(jv, ref, bound, name + ": J v against the fixture")


@pytest.mark.parametrize("name", ["default", "hands_steps"])
def test_exact_identities(model, emus, name):
    st, e = emus[name]
    ir, jc, hr, hc = e.sparsity()
    x, p = ppc.workload(name, st, model, 2200)
    x, p = x[1], p[1]
    lam, sigma, _ = ppc.factors(e.m, e.n, 41, batch=1)
    _, grad, _, jac = e.eval(x, p)
    vals = e.hess(x, p, sigma[0], lam[0])
    # sigma = 1, lambda = 0: xbar is grad f
    assert np.array_equal(e.lagrangian_grad(x, p, 1.0, np.zeros(e.m)).out, grad)
    H = np.zeros((e.n, e.n))
    H[hr, hc] = vals
    H[hc, hr] = vals
    for c in range(e.n):
        unit = np.zeros(e.n)
        unit[c] = 1.0
        d, jv = e.jac_vec(x, p, unit)
        col = np.zeros(e.m)
        col[ir[jc == c]] = jac[jc == c]
        assert np.array_equal(jv.out, col), c           # (+0.0 + J 1 + 0 J' ...: exact; a zero product adds nothing to a finite sum)
        assert d.out[0] == grad[c], c
        hv = e.hess_vec(x, p, sigma[0], lam[0], unit)
        assert np.array_equal(hv.out, H[:, c]), c


def test_either_output_of_the_jacobian_product_alone(model, emus):
    st, e = emus["hands"]
    x, p = ppc.workload("hands", st, model, 2300)
    v = np.random.RandomState(3).standard_normal(e.n)
    d, jv = e.jac_vec(x[0], p[0], v)
    d1, none = e.jac_vec(x[0], p[0], v, want_jv=False)
    none2, jv1 = e.jac_vec(x[0], p[0], v, want_dot=False)
    assert none is None and none2 is None
    assert d1.out[0] == d.out[0] and np.array_equal(jv1.out, jv.out)
    assert np.all(d1.writes == 1) and np.all(jv1.writes == 1) and d1.intact() and jv1.intact()


@pytest.mark.parametrize("name", VARIANTS)
def test_table_properties(emus, name):
    _, e = emus[name]
    ir, jc, hr, hc = e.sparsity()
    t = e.tables()
    # column directory: the CCS order itself, every position once
    assert t["jcolptr"][0] == 0 and t["jcolptr"][-1] == e.nnz and np.all(np.diff(t["jcolptr"]) >= 0)
    for c in range(e.n):
        assert np.all(jc[t["jcolptr"][c]:t["jcolptr"][c + 1]] == c)
    # row directory: every position once, the entries of a row in ascending column
    assert t["jrowptr"][0] == 0 and t["jrowptr"][-1] == e.nnz
    assert np.array_equal(np.sort(t["jrowent"]), np.arange(e.nnz))
    for i in range(e.m):
        ent = t["jrowent"][t["jrowptr"][i]:t["jrowptr"][i + 1]]
        assert np.all(ir[ent] == i) and np.all(np.diff(jc[ent]) > 0)
    # touches: every lower-triangle entry touches its row once and, off the diagonal, its column once; CCS-position order per variable
    _, hperm = e.perms()
    seen_row, seen_col = np.zeros(e.hnnz, int), np.zeros(e.hnnz, int)
    assert t["htouchptr"][0] == 0 and t["htouchptr"][-1] == e.ntouch
    for i in range(e.n):
        q = slice(t["htouchptr"][i], t["htouchptr"][i + 1])
        pos, slot, other = t["touch_pos"][q], t["touch_slot"][q], t["touch_other"][q]
        assert np.all(np.diff(pos) > 0)
        assert np.array_equal(slot, hperm[pos])
        for e_, o_ in zip(pos, other):
            if hr[e_] == i and hc[e_] == o_:
                seen_row[e_] += 1
            else:
                assert hc[e_] == i and hr[e_] == o_ and hr[e_] != hc[e_]
                seen_col[e_] += 1
    assert np.all(seen_row == 1) and np.array_equal(seen_col, (hr != hc).astype(int))
    assert np.array_equal(np.diff(t["htouchptr"]), ppc.hvp_check.touch_counts(hr, hc, e.n))
    # capacities of the kernels
    assert e.nnz <= e.ent_cap and e.m <= e.row_cap and e.ntouch <= e.touch_cap and e.n <= e.wg
    assert max(np.diff(t["jcolptr"]).max(), np.diff(t["jrowptr"]).max(), np.diff(t["htouchptr"]).max()) <= e.cnt_max
    # the device words are these directories: value index in bits 0..11, factor index above; words behind the end are empty
    w = e.device_words()
    jstage, _ = e.perms()
    assert np.array_equal(w["col_word"][:e.nnz] & 4095, jstage) and np.array_equal(w["col_word"][:e.nnz] >> 12, ir)
    assert np.array_equal(w["row_word"][:e.nnz] & 4095, jstage[t["jrowent"]]) and np.array_equal(w["row_word"][:e.nnz] >> 12, jc[t["jrowent"]])
    assert np.array_equal(w["touch_word"][:e.ntouch] & 4095, t["touch_slot"]) and np.array_equal(w["touch_word"][:e.ntouch] >> 12, t["touch_other"])
    assert not w["col_word"][e.nnz:].any() and not w["row_word"][e.nnz:].any() and not w["touch_word"][e.ntouch:].any()
    for key, ptr, count in (("col_dir", t["jcolptr"], e.n), ("row_dir", t["jrowptr"], e.m), ("var_dir", t["htouchptr"], e.n)):
        assert np.array_equal(w[key][:count] & 4095, ptr[:-1]) and np.array_equal(w[key][:count] >> 12, np.diff(ptr))
        assert not w[key][count:].any()


@pytest.mark.parametrize("name", VARIANTS)
def test_products_are_wave_order_independent(model, emus, name):
    """Groups of one phase on different waves run concurrently on the GPU: with every phase of the two programs run wave by wave in three
    orders of the four waves, the three products must be the table-order values bit for bit."""
    st, e = emus[name]
    x, p = ppc.workload(name, st, model, 2400)
    lam, sigma, v = ppc.factors(e.m, e.n, 51, batch=1)
    ref = all_products(e, x[0], p[0], sigma[0], lam[0], v[0])
    try:
        for order in (0, 1, 2):
            set_wave_order(order)
            got = all_products(e, x[0], p[0], sigma[0], lam[0], v[0])
            for a, b, what in zip(got, ref, ("xbar", "grad f . v", "J v", "H v")):
                assert np.array_equal(a, b), (order, what)
    finally:
        set_wave_order(-1)
