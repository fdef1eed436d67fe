"""What the CPU emulation tests (test_pose_kkt_hostemu.py) and the GPU tests (test_gpu_pose_kkt.py) of the pose finder's KKT chain share:
the seeded inputs, the numpy restatement of the recurrence of knot_minres.h, and the dense references.

The inputs of one settings variant come from ONE RandomState(7), drawn in this order (the order of the measurement the feature was
specified with): for scale in (0.05, 0.02): jac = scale N(0,1)^nnz, hess = scale N(0,1)^hnnz, dx in U[1, 2]^n, dc in U[1, 2]^m,
b ~ N(0,1)^(n+m), a random preconditioner in U[0.5, 2]^(n+m), S = 10^U[-3, 3]^(n+m); then for each of the three poses of
pose_products_check.workload(name, st, model, 2100): dx, dc, b.  The real value runs themselves are the caller's (the emulation's own
eval / hess on the CPU, the handle's own launches on the GPU), at the multipliers of pose_products_check.factors(m, n, 31)."""
import numpy as np

import kkt_check

WORKLOAD_SEED, FACTOR_SEED, INPUT_SEED = 2100, 31, 7
SCALES = (0.05, 0.02)


def inputs(n, m, nnz, hnnz):
    """(synthetic, real): synthetic[i] for SCALES[i] is a dict jac, hess, dx, dc, bt, bb, mt, mb, st, sb (S = diag(st, sb)); real[b] a dict
    dx, dc, bt, bb for pose b"""
    rng = np.random.RandomState(INPUT_SEED)
    synthetic = []
    for scale in SCALES:
        d = dict(jac=rng.standard_normal(nnz) * scale, hess=rng.standard_normal(hnnz) * scale, dx=rng.uniform(1, 2, n), dc=rng.uniform(1, 2, m))
        b, mv, S = rng.standard_normal(n + m), rng.uniform(0.5, 2.0, n + m), 10.0 ** rng.uniform(-3, 3, n + m)
        d.update(bt=b[:n].copy(), bb=b[n:].copy(), mt=mv[:n].copy(), mb=mv[n:].copy(), st=S[:n].copy(), sb=S[n:].copy())
        synthetic.append(d)
    real = []
    for _ in range(3):
        dx, dc, b = rng.uniform(1, 2, n), rng.uniform(1, 2, m), rng.standard_normal(n + m)
        real.append(dict(dx=dx, dc=dc, bt=b[:n].copy(), bb=b[n:].copy()))
    return synthetic, real


def rescaled(d, pat):
    """the system S K S, S b of a synthetic input (pat: hr, hc, ir, jc)"""
    hr, hc, ir, jc = pat
    st, sb = d["st"], d["sb"]
    return dict(hess=d["hess"] * st[hr] * st[hc], jac=d["jac"] * sb[ir] * st[jc], dx=d["dx"] * st ** 2, dc=d["dc"] * sb ** 2, bt=d["bt"] * st, bb=d["bb"] * sb)


def dense(n, m, pat, hess, jac, dx=None, dc=None):
    hr, hc, ir, jc = pat
    return kkt_check.dense(n, m, hr, hc, hess, ir, jc, jac, dx, dc)


def residual_2norm(n, m, pat, d, top, bottom):
    """|| K z - b ||_2 / || b ||_2 through the dense matrix"""
    K = dense(n, m, pat, d["hess"], d["jac"], d.get("dx"), d.get("dc"))
    b = np.concatenate([d["bt"], d["bb"]])
    return float(np.linalg.norm(K @ np.concatenate([top, bottom]) - b) / np.linalg.norm(b))


def numpy_diagonal(n, m, pat, hess, jac, dx, dc, floor=1e-10):
    """the diagonal in plain float64 numpy (another order of the row sums): for iteration counts, not for bits"""
    hr, hc, ir, jc = pat
    hd = np.zeros(n)
    on = hr == hc
    hd[hr[on]] = hess[on]
    top = 1.0 / np.maximum(np.abs(hd + dx), floor)
    bot = 1.0 / np.maximum(np.abs(dc + np.bincount(ir, weights=jac * jac * top[jc], minlength=m)), floor)
    return top, bot


def numpy_minres(K, b, minv, rtol, maxit):
    """(iterations, phibar / beta1, z): the recurrence of knot_minres.h in plain numpy, without fused multiply-adds"""
    n = b.size
    r1, r2 = b.copy(), b.copy()
    y = minv * r2
    beta1 = beta = np.sqrt(r2 @ y)
    oldb = dbar = epsln = 0.0
    phibar, cs, sn = beta1, -1.0, 0.0
    w, w2, z = np.zeros(n), np.zeros(n), np.zeros(n)
    for it in range(1, maxit + 1):
        v = y / beta
        y = K @ v
        if it >= 2:
            y -= (beta / oldb) * r1
        alfa = v @ y
        y -= (alfa / beta) * r2
        r1, r2 = r2, y
        y = minv * r2
        oldb = beta
        s = r2 @ y
        if not s >= 0:
            return it, np.nan, z
        beta = np.sqrt(s)
        oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
        epsln, dbar = sn * beta, -cs * beta
        gamma = max(np.sqrt(gbar * gbar + beta * beta), 2.2250738585072014e-308)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w1, w2 = w2, w
        w = (v - oldeps * w1 - delta * w2) / gamma
        z = z + phi * w
        if phibar <= rtol * beta1:
            return it, phibar / beta1, z
    return maxit, phibar / beta1, z
