"""The accuracy checks of the pose finder's products xbar = sigma grad f + J^T lambda, J v, grad f . v and H v, shared by the CPU emulation
tests (test_pose_products_hostemu.py) and the GPU tests (test_gpu_pose_products.py).

u = 2^-53, gamma_k = k u / (1 - k u) (lgrad_check.gamma).  K_c = entries of column c of jac g, K_i = entries of row i (J v) or touches of
variable i (H v), K = 81 for grad f . v.  Every product is held to two references:
  - the outputs of the SAME source (the emulation's own eval / hess; on the GPU the handle's own hipnlp_pose_eval_device and
    hipnlp_pose_eval_hess_device values) combined on the host: the same products summed in another order, 2 gamma_{K+1} sum |a| |b|;
  - the oracle (PoseOracle, AD) combined on the host: TOL sum max(1, |a|) |b| on top of that, TOL the entrywise tolerance the pose
    outputs themselves are held to (test_pose_body_hostemu.py, test_gpu_pose.py): 1e-10 for grad f and jac g, 1e-11 for the Hessian on
    the planar terrain and 1e-10 on the smooth steps."""
import numpy as np

import hvp_check
import lgrad_check

TOL_J = 1e-10
N_DOT = 81


def tol_h(name):
    return 1e-10 if name.endswith("steps") else 1e-11


def row_times(ir, jc, vals, v, m, absolute=False, floor=False):
    """sum_c J_ic v_c per row (absolute: |J| |v|; floor: max(1, |J|) |v|)"""
    vals, v = np.asarray(vals, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if floor:
        vals, v = np.maximum(1.0, np.abs(vals)), np.abs(v)
    elif absolute:
        vals, v = np.abs(vals), np.abs(v)
    return np.bincount(ir, weights=vals * v[jc], minlength=m)


def check_first_order(what, pattern, own, ora, got, sigma, lam, v):
    """pattern: (irow, jcol) of jac g; own / ora: (grad f, jac g values) of the same source / of the oracle; got: (xbar, grad f . v, J v)"""
    ir, jc = pattern
    n, m = own[0].size, lam.size
    xbar, dot, jv = got
    k_c, k_i = lgrad_check.column_counts(jc, n), np.bincount(ir, minlength=m)
    # xbar
    ref, bound = lgrad_check.own_bound(own[0], ir, jc, own[1], sigma, lam)
    lgrad_check.check(xbar, ref, bound, what + ": xbar against the same source")
    ref, bound = lgrad_check.oracle_bound(ora[0], ir, jc, ora[1], sigma, lam, k_c, TOL_J)
    lgrad_check.check(xbar, ref, bound, what + ": xbar against the oracle")
    # J v
    g2 = 2.0 * lgrad_check.gamma(k_i + 1)
    lgrad_check.check(jv, row_times(ir, jc, own[1], v, m), g2 * row_times(ir, jc, own[1], v, m, absolute=True), what + ": J v against the same source")
    lgrad_check.check(jv, row_times(ir, jc, ora[1], v, m), TOL_J * row_times(ir, jc, ora[1], v, m, floor=True) + g2 * row_times(ir, jc, ora[1], v, m, absolute=True),
                      what + ": J v against the oracle")
    # grad f . v
    gd = 2.0 * lgrad_check.gamma(N_DOT + 1)
    assert n == N_DOT
    for src, tol, label in ((own[0], 0.0, "the same source"), (ora[0], TOL_J, "the oracle")):
        ref = np.array([np.dot(src, v)])
        bound = np.array([tol * np.dot(np.maximum(1.0, np.abs(src)), np.abs(v)) + gd * np.dot(np.abs(src), np.abs(v))])
        lgrad_check.check(np.atleast_1d(dot), ref, bound, what + ": grad f . v against " + label)


def check_second_order(what, hpattern, own_vals, Href, got, v, tol):
    """hpattern: (hrow, hcol) of the lower triangle; own_vals: the same source's value run; Href: the oracle's dense Hessian; got: H v"""
    hr, hc = hpattern
    n = v.size
    k_i = hvp_check.touch_counts(hr, hc, n)
    ref, bound = hvp_check.own_bound(hr, hc, own_vals, v, k_i)
    hvp_check.check(got, ref, bound, what + ": H v against the same source")
    ref, bound = dense_hess_bound(Href, hr, hc, v, k_i, tol)
    hvp_check.check(got, ref, bound, what + ": H v against the reference Hessian")


def dense_hess_bound(Href, hr, hc, v, k_i, tol):
    """(reference, bound) from a dense symmetric Hessian: TOL sum_c max(1, |H_ic|) |v_c| + 2 gamma_{K_i+1} sum_c |H_ic| |v_c|, c over the
    handle's pattern united with the reference's non-zeros (hvp_check.oracle_bound with smooth=False scales and the tolerance given)"""
    L = np.tril(np.asarray(Href, dtype=np.float64))
    mask = L != 0.0
    mask[hr, hc] = True
    ro, co = np.nonzero(mask)
    vo = L[ro, co]
    ref = hvp_check.sym_times(ro, co, vo, v)
    bound = tol * hvp_check.sym_times(ro, co, np.maximum(1.0, np.abs(vo)), v, absolute=True) + 2.0 * hvp_check.gamma(np.asarray(k_i) + 1) * hvp_check.sym_times(ro, co, vo, v, absolute=True)
    return ref, bound


def workload(name, st, model, seed):
    """three poses (pose 0 of the *steps variants on the flanks of the first bump), lambda ~ N(0, 1)^m, sigma ~ U(0.2, 2), v ~ N(0, 1)^81 per pose"""
    from hippopt_amd.pose_settings import make_pose_workload
    from test_pose_body_hostemu import flank_points
    x, p = make_pose_workload(st, model, 3, seed)
    if name.endswith("steps"):
        flank_points(x[0], 4)
    return x, p


def factors(m, n, seed, batch=3):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((batch, m)), rng.uniform(0.2, 2.0, batch), rng.standard_normal((batch, n))
