"""The stored-values products J v, grad f . v and sigma grad f + J^T lambda (hippopt_amd/csrc/knot_jprod.h over the row and column
directories Layout::build records), run by the CPU emulation of hipnlp_jac_times_kernel / hipnlp_jac_transpose_times_kernel
(tests/jprod_emu) on a random value run: the directories cover the pattern exactly once, unit vectors give columns and rows bit for bit,
random vectors meet the rounding bounds, both jac orders give the same bits, every output is written exactly once.  CPU only."""
import numpy as np
import pytest

from hippopt_amd.kinodyn_settings import stairs_settings
from lgrad_check import check, gamma, own_bound
from test_gpu_lagrangian_grad import PLANNERS

MAKERS = dict(PLANNERS, stairs=stairs_settings)
HORIZONS = (2, 3, 4, 7)
_CACHE = {}


def emu_of(model, name, horizon, lifted, vary_first):
    """(emulation, irow, jcol) of a layout, built once"""
    from jprod_emu_lib import JprodEmu
    key = (name, horizon, lifted, vary_first)
    if key not in _CACHE:
        emu = JprodEmu(MAKERS[name](horizon, model), model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
        _CACHE[key] = (emu,) + emu.sparsity()
    return _CACHE[key]


def value_run(emu, seed):
    return np.random.RandomState(seed).standard_normal(emu.nnz)


def gradient(rng, n):
    """a random grad f: the six horizon-global variables carry no cost, the kernels do not read their elements"""
    g = rng.standard_normal(n)
    g[-6:] = 0.0
    return g


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def matrix(fn):
    for mark in (pytest.mark.parametrize("name", list(MAKERS)), pytest.mark.parametrize("horizon", HORIZONS),
                 pytest.mark.parametrize("lifted", [False, True]), pytest.mark.parametrize("vary_first", [False, True])):
        fn = mark(fn)
    return fn


@matrix
def test_directories_cover_the_pattern_exactly_once(model, name, horizon, lifted, vary_first):
    emu, ir, jc = emu_of(model, name, horizon, lifted, vary_first)
    owners, idx, row, knot, var = emu.row_directory()
    assert np.array_equal(owners, np.ones(emu.m, np.int32)), np.flatnonzero(owners != 1)[:8]
    # every pattern entry once, under its own row, with its own variable of v
    assert idx.size == emu.nnz and np.array_equal(np.sort(idx), np.arange(emu.nnz))
    assert np.array_equal(ir[idx], row) and np.array_equal(jc[idx], var)
    # ownership: the knot of the row's block — a row with entries in the blocks of knots k - 1 and k belongs to knot k; rows of both horizon
    # ends (periodicity) to the last knot; a row that reaches the horizon-global columns to knot 0
    kcol = np.minimum(jc[idx] // 189, horizon)
    for r in np.unique(row):
        sel = row == r
        ks = np.unique(kcol[sel])
        own = int(knot[sel][0])
        assert np.all(knot[sel] == own)
        if horizon in ks:
            assert own == 0 and set(ks) <= {0, horizon}
        elif ks.size == 2 and ks[1] - ks[0] == 1:
            assert own == ks[1]
        elif ks.size == 2:
            assert (ks[0], ks[1]) == (0, horizon - 1) and own == horizon - 1
        else:
            assert ks.size == 1
    # ascending column inside every row (entries of one row are consecutive)
    same = row[1:] == row[:-1]
    assert np.all(jc[idx][1:][same] > jc[idx][:-1][same])
    assert np.unique(row[np.r_[True, ~same]]).size == np.count_nonzero(np.r_[True, ~same])   # (one run per row)
    cidx, ccol, crow = emu.col_directory()
    assert cidx.size == emu.nnz and np.array_equal(np.sort(cidx), np.arange(emu.nnz))
    assert np.array_equal(ir[cidx], crow) and np.array_equal(jc[cidx], ccol)
    csame = ccol[1:] == ccol[:-1]
    assert np.all(ccol[1:] >= ccol[:-1]) and np.all(crow[1:][csame] > crow[:-1][csame])   # (column, row) order
    c = emu.counts()
    assert max(c["rows"]) <= 2 * 256 and max(c["entries"]) <= 8 * 256 and max(c["block"]) <= 7 * 256 and max(c["multipliers"]) <= 2 * 256
    assert c["other"] <= 128 and c["glob"] <= 16


@matrix
def test_unit_vectors_give_columns_and_rows_bit_for_bit(model, name, horizon, lifted, vary_first):
    emu, ir, jc = emu_of(model, name, horizon, lifted, vary_first)
    vals = value_run(emu, 11 + horizon)
    v = np.zeros(emu.n)
    for c in range(emu.n):
        v[c] = 1.0
        jv, _, _, _ = emu.jac_times(vals, v)
        v[c] = 0.0
        want = np.zeros(emu.m)
        want[ir[jc == c]] = vals[jc == c]
        assert np.array_equal(bits(jv), bits(want)), ("J e_c", c)
    lam = np.zeros(emu.m)
    order = np.argsort(ir, kind="stable")
    starts = np.searchsorted(ir[order], np.arange(emu.m + 1))
    for i in range(emu.m):
        lam[i] = 1.0
        out, _ = emu.jac_transpose_times(vals, lam)
        lam[i] = 0.0
        sel = order[starts[i]:starts[i + 1]]
        want = np.zeros(emu.n)
        want[jc[sel]] = vals[sel]
        assert np.array_equal(bits(out), bits(want)), ("J^T e_i", i)


@matrix
def test_random_vectors_meet_the_rounding_bounds(model, name, horizon, lifted, vary_first):
    emu, ir, jc = emu_of(model, name, horizon, lifted, vary_first)
    rng = np.random.RandomState(23 + horizon)
    vals, grad, v, lam = value_run(emu, 5), gradient(rng, emu.n), rng.standard_normal(emu.n), rng.standard_normal(emu.m)
    what = "%s N=%d lifted=%s vary_first=%s" % (name, horizon, lifted, vary_first)
    jv, dot, jw, dw = emu.jac_times(vals, v, grad=grad)
    assert np.array_equal(jw, np.ones(emu.m, np.int32)) and dw == 1
    k_i = np.bincount(ir, minlength=emu.m)
    ref = np.bincount(ir, weights=vals * v[jc], minlength=emu.m)
    s = np.bincount(ir, weights=np.abs(vals) * np.abs(v[jc]), minlength=emu.m)
    check(jv, ref, 2.0 * gamma(k_i + 1) * s, what + " J v")
    dref, dbound = float(np.dot(grad, v)), 2.0 * float(gamma(emu.n + 1)) * float(np.dot(np.abs(grad), np.abs(v)))
    print("%s grad.v: |dot - ref| = %.3e, bound %.3e" % (what, abs(dot - dref), dbound))
    assert abs(dot - dref) <= dbound
    for sigma in (1.0, 0.0, float(rng.uniform(0.1, 3.0))):
        out, w = emu.jac_transpose_times(vals, lam, sigma=sigma, grad=grad)
        assert np.array_equal(w, np.ones(emu.n, np.int32))
        ref, bound = own_bound(grad, ir, jc, vals, sigma, lam)
        check(out, ref, bound, what + " sigma=%g" % sigma)
    out, _ = emu.jac_transpose_times(vals, lam)   # no gradient: J^T lam
    ref, bound = own_bound(np.zeros(emu.n), ir, jc, vals, 0.0, lam)
    check(out, ref, bound, what + " no gradient")


@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("horizon", HORIZONS)
@pytest.mark.parametrize("name", list(MAKERS))
def test_ccs_and_varying_first_give_the_same_bits(model, name, horizon, lifted):
    ccs, ir_c, jc_c = emu_of(model, name, horizon, lifted, False)
    vf, ir_v, jc_v = emu_of(model, name, horizon, lifted, True)
    assert not (np.array_equal(ir_c, ir_v) and np.array_equal(jc_c, jc_v))   # (the two orders of a block really differ)
    key_c, key_v = jc_c.astype(np.int64) * ccs.m + ir_c, jc_v.astype(np.int64) * ccs.m + ir_v
    assert np.all(np.diff(key_c) > 0)   # CCS
    perm = np.searchsorted(key_c, key_v)
    assert np.array_equal(key_c[perm], key_v)
    rng = np.random.RandomState(77)
    vals, grad, v, lam = value_run(ccs, 6), gradient(rng, ccs.n), rng.standard_normal(ccs.n), rng.standard_normal(ccs.m)
    a_jv, a_dot, _, _ = ccs.jac_times(vals, v, grad=grad)
    b_jv, b_dot, _, _ = vf.jac_times(vals[perm], v, grad=grad)
    assert np.array_equal(bits(a_jv), bits(b_jv)) and bits([a_dot])[0] == bits([b_dot])[0]
    a, _ = ccs.jac_transpose_times(vals, lam, sigma=0.75, grad=grad)
    b, _ = vf.jac_transpose_times(vals[perm], lam, sigma=0.75, grad=grad)
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name,horizon", [("periodic", 2), ("periodic", 3), ("single", 4), ("stairs", 7)])
def test_every_output_is_written_exactly_once_and_a_missing_one_is_left_alone(model, name, horizon):
    for lifted in (False, True):
        emu, _, _ = emu_of(model, name, horizon, lifted, False)
        rng = np.random.RandomState(3)
        vals, grad, v = value_run(emu, 8), gradient(rng, emu.n), rng.standard_normal(emu.n)
        jv, dot, jw, dw = emu.jac_times(vals, v, grad=grad)
        assert np.array_equal(jw, np.ones(emu.m, np.int32)) and dw == 1 and np.all(np.isfinite(jv)) and np.isfinite(dot)
        jv2, dot2, jw2, dw2 = emu.jac_times(vals, v, grad=grad, want_jv=False)
        assert jv2 is None and not jw2.any() and dw2 == 1 and bits([dot2])[0] == bits([dot])[0]
        jv3, dot3, jw3, dw3 = emu.jac_times(vals, v)
        assert dot3 is None and dw3 == 0 and np.array_equal(bits(jv3), bits(jv))
        out, w = emu.jac_transpose_times(vals, rng.standard_normal(emu.m))
        assert np.array_equal(w, np.ones(emu.n, np.int32)) and np.all(np.isfinite(out))
