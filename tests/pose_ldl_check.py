"""What the CPU emulation tests (test_pose_ldl_hostemu.py) and the GPU tests (test_gpu_pose_ldl.py) of the pose finder's dense L D L^T share:
the systems (pose_kkt_check.inputs and its dense K, unchanged), the backward error and its bound, the reference inertia, the ladder walked
in numpy, and the cases that are singular or not finite.

The bound on the normwise backward error eta = |K z - b|_inf / (|K|_inf |z|_inf + |b|_inf) is max(16 eta_numpy, N 2^-53), eta_numpy that of
numpy.linalg.solve (LU with partial pivoting) on the same dense system: 16 is a margin for another pivoting strategy, not a measurement.

The reference inertia is the sign count of numpy.linalg.eigvalsh(K), used only where the smallest |eigenvalue| exceeds 1e-8 |K|_2.  The
rescaled system S K S (cond about 1e12) cannot satisfy that by construction; its inertia is that of K itself by Sylvester's law (S is a
positive diagonal), so its reference — and the precondition — are taken on K."""
import numpy as np

import pose_kkt_check as pkc
import pose_products_check as ppc

U = 2.0 ** -53
DELTA_INIT, KAPPA = 1e-4, 8.0
_REAL = {}


def eta(K, z, b):
    return float(np.linalg.norm(K @ z - b, np.inf) / (np.linalg.norm(K, np.inf) * np.linalg.norm(z, np.inf) + np.linalg.norm(b, np.inf)))


def eta_bound(K, b):
    """(the bound, numpy's own eta)"""
    ref = eta(K, np.linalg.solve(K, b), b)
    return max(16.0 * ref, K.shape[0] * U), ref


def sign_counts(K):
    """((positive, negative, zero), smallest |eigenvalue| / |K|_2)"""
    ev = np.linalg.eigvalsh(K)
    return (int((ev > 0).sum()), int((ev < 0).sum()), int((ev == 0).sum())), float(np.abs(ev).min() / np.abs(ev).max())


def real_runs(model, name, variants, e):
    """the real systems of a variant: for each of the three workload poses a dict hess, jac, dx, dc, bt, bb — the value runs from the CPU
    emulation of the pose kernels (tests/pose_products_emu), computed once"""
    from pose_products_emu_lib import PoseProductsEmu
    if name not in _REAL:
        st = variants(model)[name]
        pe = PoseProductsEmu(st, model)
        x, p = ppc.workload(name, st, model, pkc.WORKLOAD_SEED)
        lam, sigma, _ = ppc.factors(e.m, e.n, pkc.FACTOR_SEED)
        _, real = pkc.inputs(e.n, e.m, e.nnz, e.hnnz)
        _REAL[name] = [dict(real[b], jac=pe.eval(x[b], p[b])[3], hess=pe.hess(x[b], p[b], sigma[b], lam[b])) for b in range(3)]
    return _REAL[name]


def synthetic_systems(e, pat):
    """[(label, system, the system whose eigenvalues give the reference inertia)]: the two synthetic inputs and the first one rescaled"""
    syn, _ = pkc.inputs(e.n, e.m, e.nnz, e.hnnz)
    return [("synthetic 0.05", syn[0], syn[0]), ("synthetic 0.02", syn[1], syn[1]), ("rescaled", pkc.rescaled(syn[0], pat), syn[0])]


def dense_of(e, pat, d, delta=0.0, dx="own", dc="own"):
    dx = d.get("dx") if isinstance(dx, str) else dx
    dc = d.get("dc") if isinstance(dc, str) else dc
    K = pkc.dense(e.n, e.m, pat, d["hess"], d["jac"], dx, dc)
    if delta:
        K = K.copy()
        K[np.arange(e.n), np.arange(e.n)] += delta
    return K


def rhs_of(d):
    return np.concatenate([d["bt"], d["bb"]])


def indefinite(d):
    """the ladder's case: the synthetic system with dx negated, so that H + diag dx is indefinite"""
    return dict(d, dx=-d["dx"])


def numpy_ladder(e, pat, d, delta_init=DELTA_INIT, kappa=KAPPA, cap=16):
    """(tries, delta) of the first try whose eigenvalues count (81, m, 0): try 0 has delta 0, try t >= 1 delta_init kappa^(t-1) by one
    rounded product per try; None where `cap` tries do not reach it"""
    delta = 0.0
    for t in range(cap + 1):
        if t >= 1:
            delta = delta_init if t == 1 else delta * kappa
        counts, _ = sign_counts(dense_of(e, pat, d, delta))
        if counts == (e.n, e.m, 0):
            return t, delta
    return None


def singular(d):
    """all-zero jac values (with dc left out: a zero bottom block)"""
    return dict(d, jac=np.zeros_like(d["jac"]))


def with_nan(d, at=5):
    h = d["hess"].copy()
    h[at] = np.nan
    return dict(d, hess=h)


def pivot_kinds(pivots):
    """(2x2 pivots, 1x1 pivots with an interchange, 1x1 pivots without) of a pivot vector in LAPACK's convention"""
    two = one_swap = one_stay = 0
    k, N = 0, len(pivots)
    while k < N:
        if pivots[k] < 0:
            two += 1
            k += 2
        else:
            if pivots[k] == k + 1:
                one_stay += 1
            else:
                one_swap += 1
            k += 1
    return two, one_swap, one_stay
