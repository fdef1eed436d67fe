"""Host references of the KKT operator  K = [[H + diag dx, J^T], [J, -diag dc]]  (CPU emulation and GPU tests alike): the dense matrix
from the two patterns and value runs, the product through the patterns, and the exactly rounded fused multiply-add of the diagonal terms
(fractions.Fraction is exact, float() rounds to nearest even: what one fma instruction returns)."""
from fractions import Fraction

import numpy as np

from hvp_check import sym_times


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dense(n, m, hr, hc, hv, ir, jc, jv, dx=None, dc=None):
    """K [n + m, n + m] from the lower triangle (hr, hc, hv) of H and the triplets (ir, jc, jv) of J; the diagonal of the (1, 1) block is
    H_cc + dx_c in one float64 addition"""
    K = np.zeros((n + m, n + m))
    K[hr, hc] = hv
    K[hc, hr] = hv
    K[n + np.asarray(ir), jc] = jv
    K[jc, n + np.asarray(ir)] = jv
    if dx is not None:
        K[np.arange(n), np.arange(n)] += dx
    if dc is not None:
        K[n + np.arange(m), n + np.arange(m)] = -np.asarray(dc)
    return K


def apply(n, m, hr, hc, hv, ir, jc, jv, dx, dc, v, w, absolute=False):
    """(top, bottom) = K [v; w] in float64 on the host through the patterns; absolute: |K| [|v|; |w|]"""
    a = np.abs if absolute else (lambda t: t)
    hv, jv, v, w = a(np.asarray(hv)), a(np.asarray(jv)), a(np.asarray(v)), a(np.asarray(w))
    top = sym_times(hr, hc, hv, v) + np.bincount(jc, weights=jv * w[ir], minlength=n)
    bottom = np.bincount(ir, weights=jv * v[jc], minlength=m)
    if dx is not None:
        top = top + a(np.asarray(dx)) * v
    if dc is not None:
        bottom = bottom + (a(np.asarray(dc)) * w if absolute else -np.asarray(dc) * w)
    return top, bottom


def exact_fma(a, x, s):
    """round(a x + s) elementwise, one rounding"""
    return np.array([float(Fraction(float(ai)) * Fraction(float(xi)) + Fraction(float(si))) for ai, xi, si in zip(a, x, s)])
