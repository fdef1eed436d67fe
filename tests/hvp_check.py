"""The error bounds of the Hessian-vector product y = H(x, sigma, lambda) v (CPU emulation and GPU tests alike).

u = 2^-53, gamma_k = k u / (1 - k u), K_i = touches of variable i (entries of the lower triangle with i as row or column; + 1 where the
variable has a periodicity-coupling term), S_i = sum_c |H_ic| |v_c|.
  - against the same handle's own eval_hess_device values multiplied on the host: |y_i - ref_i| <= 2 gamma_{K_i+1} S_i (the same products
    summed in another order, each side rounding);
  - against the oracle (forward-over-forward AD): TOL sum_c s_ic |v_c| + 2 gamma_{K_i+1} S_i, H from the oracle, c over the handle's
    pattern united with the oracle's entries; s_ic = max(1, |H_ic|), TOL = 1e-11 on the planar terrain; s_ic = max(1, |H_ic|,
    sqrt(|H_ii H_cc|)), TOL = 1e-9 on the smooth terrain: the entrywise tolerances and scales the Hessian itself is held to
    (tests/hess_util.py), summed along a row."""
import numpy as np

U = 2.0 ** -53
TOL_PLANAR, TOL_SMOOTH = 1e-11, 1e-9


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def sym_times(ir, jc, vals, v, absolute=False):
    """H v for a symmetric H given by its lower triangle (float64 on the host); absolute: |H| |v|"""
    ir, jc = np.asarray(ir), np.asarray(jc)
    vals, v = np.asarray(vals, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if absolute:
        vals, v = np.abs(vals), np.abs(v)
    off = ir != jc
    return np.bincount(ir, weights=vals * v[jc], minlength=v.size) + np.bincount(jc[off], weights=vals[off] * v[ir[off]], minlength=v.size)


def touch_counts(ir, jc, n):
    """K_i of a lower-triangle pattern: a coupling entry counts for both of its variables like any off-diagonal entry"""
    ir, jc = np.asarray(ir), np.asarray(jc)
    off = ir != jc
    return np.bincount(ir, minlength=n) + np.bincount(jc[off], minlength=n)


def own_bound(ir, jc, vals, v, k_i):
    """(reference, bound) from a handle's own Hessian values"""
    return sym_times(ir, jc, vals, v), 2.0 * gamma(np.asarray(k_i) + 1) * sym_times(ir, jc, vals, v, absolute=True)


def oracle_bound(iro, jco, valo, ir, jc, v, k_i, smooth):
    """(reference, bound) from the oracle's Hessian (iro, jco, valo: lower triangle, no duplicates); (ir, jc): the handle's pattern"""
    n = v.size
    iro, jco, valo = np.asarray(iro, dtype=np.int64), np.asarray(jco, dtype=np.int64), np.asarray(valo, dtype=np.float64)
    assert np.all(iro >= jco) and np.unique(iro * n + jco).size == iro.size
    ref = sym_times(iro, jco, valo, v)
    s_abs = sym_times(iro, jco, valo, v, absolute=True)
    # the union of the two patterns: entries of the handle's pattern the oracle does not list are zeros there
    extra = np.setdiff1d(np.asarray(ir, dtype=np.int64) * n + np.asarray(jc, dtype=np.int64), iro * n + jco)
    ru, cu = np.concatenate([iro, extra // n]), np.concatenate([jco, extra % n])
    hu = np.concatenate([valo, np.zeros(extra.size)])
    scale = np.maximum(1.0, np.abs(hu))
    if smooth:
        diag = np.zeros(n)
        d = iro == jco
        diag[iro[d]] = np.abs(valo[d])
        scale = np.maximum(scale, np.sqrt(diag[ru] * diag[cu]))
    tol = TOL_SMOOTH if smooth else TOL_PLANAR
    return ref, tol * sym_times(ru, cu, scale, v, absolute=True) + 2.0 * gamma(np.asarray(k_i) + 1) * s_abs


def full_multipliers(lam, kept):
    """lambda of a (possibly lifted) handle on the rows of the full subject_to list: zero on the rows lifted into bounds"""
    kept = np.asarray(kept)
    out = np.zeros(kept.size)
    out[kept >= 0] = lam[kept[kept >= 0]]
    return out


def check(y, ref, bound, what):
    """print the worst ratio |y - ref| / bound, then assert the bound entrywise"""
    err = np.abs(y - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print("%s: max |y - ref| = %.3e, worst ratio to the bound %.3e (variable %d)" % (what, np.nanmax(err), np.nanmax(ratio), int(np.nanargmax(ratio))))
    assert np.all(err <= bound), (what, int(np.argmax(~(err <= bound))), float(np.nanmax(ratio)))


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if np.size(a) else 0.0
