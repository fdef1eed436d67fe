"""The error bounds of the Lagrangian gradient xbar = sigma grad f + J^T lambda (CPU emulation and GPU tests alike).

u = 2^-53, gamma_k = k u / (1 - k u), K_c = entries of jac g in column c, S_c = |sigma| |grad f_c| + sum_i |lambda_i| |J_ic|.
  - against outputs of the same handle summed on the host: |xbar_c - ref_c| <= 2 gamma_{K_c+1} S_c (the same K_c + 1 products summed in
    another order, each side rounding);
  - against the oracle (forward AD), combined on the host: TOL (|sigma| max(1, |grad f_c|) + sum_i |lambda_i| max(1, |J_ic|)) + 2 gamma_{K_c+1} S_c,
    grad f and J from the oracle, TOL the entrywise tolerance of grad f / jac g against the oracle (1e-11 planar, 1e-9 smooth terrain)."""
import numpy as np

U = 2.0 ** -53
TOL_PLANAR, TOL_SMOOTH = 1e-11, 1e-9


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def column_counts(jcol, n):
    """K_c of a pattern (column indices of its entries)"""
    return np.bincount(np.asarray(jcol), minlength=n)


def combine(grad, irow, jcol, jac, sigma, lam):
    """(sigma grad + J^T lam, S) on the host"""
    n = grad.size
    ref = sigma * grad + np.bincount(jcol, weights=lam[irow] * jac, minlength=n)
    s = abs(sigma) * np.abs(grad) + np.bincount(jcol, weights=np.abs(lam[irow]) * np.abs(jac), minlength=n)
    return ref, s


def own_bound(grad, irow, jcol, jac, sigma, lam):
    """(reference, bound) from a handle's own outputs"""
    ref, s = combine(grad, irow, jcol, jac, sigma, lam)
    return ref, 2.0 * gamma(column_counts(jcol, grad.size) + 1) * s


def oracle_bound(grado, iro, jco, jaco, sigma, lam_full, k_c, tol):
    """(reference, bound) from the oracle's grad f and jac g (full NLP: lam_full has a zero at every lifted row); k_c of the handle's pattern"""
    ref, s = combine(grado, iro, jco, jaco, sigma, lam_full)
    t = abs(sigma) * np.maximum(1.0, np.abs(grado)) + np.bincount(jco, weights=np.abs(lam_full[iro]) * np.maximum(1.0, np.abs(jaco)), minlength=grado.size)
    return ref, tol * t + 2.0 * gamma(np.asarray(k_c) + 1) * s


def full_multipliers(lam, kept):
    """lambda of a (possibly lifted) handle on the rows of the full subject_to list: zero on the rows lifted into bounds"""
    kept = np.asarray(kept)
    out = np.zeros(kept.size)
    out[kept >= 0] = lam[kept[kept >= 0]]
    return out


def check(xbar, ref, bound, what):
    """print the worst ratio |xbar - ref| / bound, then assert the bound entrywise"""
    err = np.abs(xbar - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print("%s: max |xbar - ref| = %.3e, worst ratio to the bound %.3e (column %d)" % (what, err.max(), ratio.max(), int(np.argmax(ratio))))
    assert np.all(err <= bound), (what, int(np.argmax(ratio)), float(ratio.max()))
