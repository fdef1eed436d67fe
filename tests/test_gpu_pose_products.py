"""GPU: the pose finder's products in one launch each — xbar = sigma grad f + J^T lambda (hipnlp_pose_eval_lagrangian_grad_device), J v and
grad f . v (hipnlp_pose_eval_jac_vec_device), H v (hipnlp_pose_eval_hess_vec_device) — and hippopt_amd.autograd.PoseNLP built on them.
The accuracy checks are those of the CPU emulation (tests/pose_products_check.py), "the same source" being the handle's own
hipnlp_pose_eval_device / hipnlp_pose_eval_hess_device outputs; every figure is printed before it is asserted."""
import ctypes
import math

import numpy as np
import pytest

import pose_products_check as ppc
from hippopt_amd.pose_settings import make_pose_workload
from test_pose_body_hostemu import VARIANTS, variants

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def guarded(shape, guard=64):
    """(buffer, view of its body): a NaN-filled destination between two runs of guard words"""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float64, device="cuda")
    buf[:guard] = 1234.5
    buf[guard + n:] = 1234.5
    return buf, buf[guard:guard + n].view(*shape)


def guards_intact(buf, guard=64):
    h = buf.cpu().numpy()
    return bool(np.all(h[:guard] == 1234.5) and np.all(h[-guard:] == 1234.5))


class Products:
    """every product and every dense output of one handle at (x, sigma, lam, v), as numpy arrays; destinations between guard words"""

    def __init__(self, eng, x, sigma, lam, v):
        import torch
        B = eng.batch
        xd, sd, ld, vd = dev(x), dev(sigma), dev(lam), dev(v)
        hr, hc = eng.hess_sparsity()
        f, grad, g, jac = (torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((B,), (B, eng.n), (B, eng.m), (B, eng.nnz)))
        vals = torch.full((B, hr.size), float("nan"), dtype=torch.float64, device="cuda")
        eng.eval_device(xd.data_ptr(), f.data_ptr(), grad.data_ptr(), g.data_ptr(), jac.data_ptr(), stream=_stream())
        eng.eval_hess_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), vals.data_ptr(), stream=_stream())
        bufs = [guarded((B, eng.n)), guarded((B,)), guarded((B, eng.m)), guarded((B, eng.n))]
        eng.eval_lagrangian_grad_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), bufs[0][1].data_ptr(), stream=_stream())
        eng.eval_jac_vec_device(xd.data_ptr(), vd.data_ptr(), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), stream=_stream())
        eng.eval_hess_vec_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), vd.data_ptr(), bufs[3][1].data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        self.guards = all(guards_intact(b[0]) for b in bufs)
        self.f, self.grad, self.g, self.jac, self.vals = (t.cpu().numpy() for t in (f, grad, g, jac, vals))
        self.xbar, self.dot, self.jv, self.hv = (b[1].cpu().numpy() for b in bufs)
        self.hr, self.hc = hr, hc


@pytest.mark.parametrize("name", VARIANTS)
def test_products_match_own_outputs_and_oracle(model, name):
    from hippopt_amd.hipnlp import HipPose
    from oracle_lib import PoseOracle
    st = variants(model)[name]
    x, p = ppc.workload(name, st, model, 2100)
    eng, o = HipPose(st, model, batch=3), PoseOracle(st, model)
    eng.set_params(p)
    lam, sigma, v = ppc.factors(eng.m, eng.n, 31)
    ir, jc = eng.sparsity()
    r = Products(eng, x, sigma, lam, v)
    assert r.guards
    for b in range(3):
        _, grado, _, jaco = o.eval(x[b], p[b])
        ppc.check_first_order("%s pose %d" % (name, b), (ir, jc), (r.grad[b], r.jac[b]), (grado, jaco), (r.xbar[b], r.dot[b], r.jv[b]), float(sigma[b]), lam[b], v[b])
        Href = o.hess(x[b], p[b], float(sigma[b]), lam[b])
        ppc.check_second_order("%s pose %d" % (name, b), (r.hr, r.hc), r.vals[b], Href, r.hv[b], v[b], ppc.tol_h(name))


def test_batch_positions_give_the_same_bits_and_guards_hold(model):
    """1 300 poses, one more round than the 1 280 workgroups resident at five per CU; three distinct poses cycled"""
    from hippopt_amd.hipnlp import HipPose
    st = variants(model)["default"]
    B = 1300
    x3, p3 = make_pose_workload(st, model, 3, 2500)
    eng = HipPose(st, model, batch=B)
    lam3, sigma3, v3 = ppc.factors(eng.m, eng.n, 61)
    cyc = np.arange(B) % 3
    eng.set_params(p3[cyc])
    r = Products(eng, x3[cyc], sigma3[cyc], lam3[cyc], v3[cyc])
    assert r.guards
    for what, a in (("xbar", r.xbar), ("grad f . v", r.dot), ("J v", r.jv), ("H v", r.hv)):
        assert np.all(np.isfinite(a)), what
        assert np.array_equal(bits(a), bits(a[:3][cyc])), what


def _fma():
    """a correctly rounded fused multiply-add on the host: math.fma (Python >= 3.13), else the C library's"""
    if hasattr(math, "fma"):
        return math.fma
    try:
        fn = ctypes.CDLL("libm.so.6").fma
    except (OSError, AttributeError):
        return None
    fn.restype, fn.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    return lambda a, b, c: fn(a, b, c)


@pytest.mark.parametrize("name", ["default", "hands_steps"])
def test_cross_kernel_consistency(model, name):
    """H v of the one launch is, bit for bit, the sum of the handle's own hipnlp_pose_eval_hess_device values in table order (per variable
    the entries of the lower triangle that have it as row or column, in CCS order, one fused multiply-add each, from +0.0), summed on the
    host with math.fma or the C library's fma; a host with neither holds it to the own bound of pose_products_check instead.  J v with
    v = e_c is the handle's own column c of jac g bitwise, grad f . e_c its own grad f_c."""
    from hippopt_amd.hipnlp import HipPose
    st = variants(model)[name]
    x, p = ppc.workload(name, st, model, 2600)
    eng = HipPose(st, model, batch=3)
    eng.set_params(p)
    lam, sigma, v = ppc.factors(eng.m, eng.n, 71)
    r = Products(eng, x, sigma, lam, v)
    fma = _fma()
    if fma is None:
        for b in range(3):
            ref, bound = ppc.hvp_check.own_bound(r.hr, r.hc, r.vals[b], v[b], ppc.hvp_check.touch_counts(r.hr, r.hc, eng.n))
            ppc.hvp_check.check(r.hv[b], ref, bound, "%s pose %d: H v against own values (no host fma)" % (name, b))
    else:
        for b in range(3):
            y = np.zeros(eng.n)
            for i in range(eng.n):
                acc = 0.0
                for e in np.flatnonzero((r.hr == i) | (r.hc == i)):
                    acc = fma(float(r.vals[b, e]), float(v[b, r.hc[e] if r.hr[e] == i else r.hr[e]]), acc)
                y[i] = acc
            assert np.array_equal(bits(r.hv[b]), bits(y)), (b, int(np.argmax(r.hv[b] != y)))
    # unit directions: the columns of the handle's own jac g and the elements of its own grad f (three columns per launch, one per pose)
    ir, jc = eng.sparsity()
    for c0 in range(0, eng.n, 3):
        cols = [min(c0 + b, eng.n - 1) for b in range(3)]
        unit = np.zeros((3, eng.n))
        unit[np.arange(3), cols] = 1.0
        q = Products(eng, x, sigma, lam, unit)
        for b, c in enumerate(cols):
            col = np.zeros(eng.m)
            col[ir[jc == c]] = r.jac[b][jc == c]
            assert np.array_equal(q.jv[b], col), (b, c)
            assert q.dot[b] == r.grad[b, c], (b, c)


def test_error_codes_and_non_finite_inputs(model):
    import torch
    from hippopt_amd.hipnlp import HipPose, HipNlpError
    st = variants(model)["default"]
    B = 3
    x, p = make_pose_workload(st, model, B, 2700)
    eng = HipPose(st, model, batch=B)
    lam, sigma, v = ppc.factors(eng.m, eng.n, 81)
    xd, sd, ld, vd = dev(x), dev(sigma), dev(lam), dev(v)
    out, dot, jv = (torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((B, eng.n), (B,), (B, eng.m)))
    X, S, L, V, O, D, J = (t.data_ptr() for t in (xd, sd, ld, vd, out, dot, jv))
    calls = {"lgrad": (eng.eval_lagrangian_grad_device, (X, S, L, O)), "jvp": (eng.eval_jac_vec_device, (X, V, D, J)), "hvp": (eng.eval_hess_vec_device, (X, S, L, V, O))}
    for what, (fn, args) in calls.items():          # before set_params
        with pytest.raises(HipNlpError) as e:
            fn(*args)
        assert e.value.code == -4, what             # HIPNLP_E_PARAMS
    eng.set_params(p)
    for what, (fn, args) in calls.items():          # a null pointer in every required position
        required = range(len(args)) if what != "jvp" else range(2)
        for k in required:
            with pytest.raises(HipNlpError) as e:
                fn(*[0 if i == k else a for i, a in enumerate(args)])
            assert e.value.code == -1, (what, k)    # HIPNLP_E_INVALID
    with pytest.raises(HipNlpError) as e:
        eng.eval_jac_vec_device(X, V, 0, 0)         # both destinations null
    assert e.value.code == -1
    lib = eng.lib
    vp = ctypes.c_void_p
    assert lib.hipnlp_pose_eval_lagrangian_grad_device(None, vp(X), vp(S), vp(L), vp(O), None) == -1
    assert lib.hipnlp_pose_eval_jac_vec_device(None, vp(X), vp(V), vp(D), vp(J), None) == -1
    assert lib.hipnlp_pose_eval_hess_vec_device(None, vp(X), vp(S), vp(L), vp(V), vp(O), None) == -1
    # either destination of the Jacobian product alone: the same bits
    eng.eval_jac_vec_device(X, V, D, J, stream=_stream())
    d2, j2 = torch.full_like(dot, float("nan")), torch.full_like(jv, float("nan"))
    eng.eval_jac_vec_device(X, V, d2.data_ptr(), 0, stream=_stream())
    eng.eval_jac_vec_device(X, V, 0, j2.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    assert torch.equal(d2.view(torch.int64), dot.view(torch.int64)) and torch.equal(j2.view(torch.int64), jv.view(torch.int64))
    # an x with a NaN: the pose's outputs are not finite, the other poses' are
    xn = x.copy()
    xn[1, 52] = np.nan                              # (a component of the base quaternion: every kinematic entry of jac g and of H depends on it)
    r = Products(eng, xn, sigma, lam, v)
    for what, a in (("xbar", r.xbar), ("J v", r.jv), ("H v", r.hv)):
        assert np.isnan(a[1]).any(), what
        assert np.all(np.isfinite(a[[0, 2]])), what


def _pose_nlp(model, name, B, seed):
    from hippopt_amd.autograd import PoseNLP
    st = variants(model)[name]
    x, p = make_pose_workload(st, model, B, seed)
    nlp = PoseNLP(st, model, batch=B)
    nlp.set_params(p)
    return nlp, x, p


def test_torch_first_derivatives(model):
    import torch
    nlp, x, _ = _pose_nlp(model, "hands", 3, 2800)
    rng = np.random.RandomState(5)
    a, w = 0.37, dev(rng.standard_normal((3, nlp.m)))
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    f, g = nlp(xt)
    assert f.shape == (3,) and g.shape == (3, nlp.m)
    (a * f.sum() + (w * g).sum()).backward()
    ref = nlp.lagrangian_gradient(xt.detach(), a, w)
    assert torch.equal(xt.grad.view(torch.int64), ref.view(torch.int64))
    # the methods are the raw launches
    r = Products(nlp.engine, x, np.full(3, a), w.cpu().numpy(), rng.standard_normal((3, nlp.n)))
    assert np.array_equal(bits(ref.cpu().numpy()), bits(r.xbar))
    assert np.array_equal(bits(f.detach().cpu().numpy()), bits(r.f)) and np.array_equal(bits(g.detach().cpu().numpy()), bits(r.g))


def test_torch_second_derivatives_of_a_quadratic_loss(model):
    """loss = sum f^2 + sum g^2: gx = 2 f grad f + 2 J^T g recorded under create_graph, then d/dx (gx . u) = H(2 f, 2 g) u + 2 (grad f . u) grad f
    + 2 J^T (J u) — one hvp launch for x, one jvp launch for sigma and lam, one more Lagrangian gradient through nlp(x).  Held to the host
    combination of the handle's own dense outputs: H from hipnlp_pose_eval_hess_device at (2 f, 2 g) (H is linear in sigma and lambda:
    2 f H_f + 2 H(0, g)), grad f and jac g from hipnlp_pose_eval_device.  Bound, term by term: the own bound of H u; the own bound of the
    Lagrangian gradient at the factors the launch saw; |grad f_c| 2 b_dot + sum_i |J_ic| 2 b_Jv,i for the factors' own bounds; and two
    roundings of the final sum."""
    import torch
    for name in ("default", "hands_steps"):
        nlp, x, _ = _pose_nlp(model, name, 3, 2900)
        eng = nlp.engine
        u = np.random.RandomState(9).standard_normal((3, nlp.n))
        ut = dev(u)
        xt = torch.tensor(x, device="cuda", requires_grad=True)
        f, g = nlp(xt)
        (gx,) = torch.autograd.grad((f ** 2).sum() + (g ** 2).sum(), xt, create_graph=True)
        assert gx.requires_grad
        (h,) = torch.autograd.grad((gx * ut).sum(), xt)
        h = h.cpu().numpy()
        fh, gh = f.detach().cpu().numpy(), g.detach().cpu().numpy()
        r = Products(eng, x, 2.0 * fh, 2.0 * gh, u)
        assert np.array_equal(bits(gx.detach().cpu().numpy()), bits(r.xbar))
        ir, jc = eng.sparsity()
        k_i = ppc.hvp_check.touch_counts(r.hr, r.hc, nlp.n)
        k_r = np.bincount(ir, minlength=nlp.m)
        for b in range(3):
            hu, b_h = ppc.hvp_check.own_bound(r.hr, r.hc, r.vals[b], u[b], k_i)
            dot_h = float(np.dot(r.grad[b], u[b]))
            b_dot = 2.0 * ppc.lgrad_check.gamma(ppc.N_DOT + 1) * float(np.dot(np.abs(r.grad[b]), np.abs(u[b])))
            jv_h = ppc.row_times(ir, jc, r.jac[b], u[b], nlp.m)
            b_jv = 2.0 * ppc.lgrad_check.gamma(k_r + 1) * ppc.row_times(ir, jc, r.jac[b], u[b], nlp.m, absolute=True)
            lg, b_lg = ppc.lgrad_check.own_bound(r.grad[b], ir, jc, r.jac[b], 2.0 * dot_h, 2.0 * jv_h)
            b_fac = np.abs(r.grad[b]) * 2.0 * b_dot + np.bincount(jc, weights=np.abs(r.jac[b]) * 2.0 * b_jv[ir], minlength=nlp.n)
            # (the launch saw factors within b_dot / b_jv of the host's: its own bound is taken at the larger magnitudes)
            _, b_lg_hi = ppc.lgrad_check.own_bound(r.grad[b], ir, jc, r.jac[b], 2.0 * (abs(dot_h) + b_dot), 2.0 * (np.abs(jv_h) + b_jv))
            ref = hu + lg
            bound = b_h + np.maximum(b_lg, b_lg_hi) + b_fac + 2.0 * U * (np.abs(hu) + np.abs(lg))
            ppc.lgrad_check.check(h[b], ref, bound, "%s pose %d: double backward of the quadratic loss" % (name, b))
        # sigma and lam that require grad: the derivatives are grad f . w and J w, bit for bit the raw launch
        sg = dev(np.full(3, 0.7)).requires_grad_()
        lm = dev(2.0 * gh).requires_grad_()
        out = nlp.lagrangian_gradient(xt.detach(), sg, lm)
        ds, dl = torch.autograd.grad((out * ut).sum(), (sg, lm))
        dot, jv = nlp.jacobian_vector_product(xt.detach(), ut)
        assert torch.equal(ds.view(torch.int64), dot.view(torch.int64)) and torch.equal(dl.view(torch.int64), jv.view(torch.int64))
        assert np.array_equal(bits(dot.cpu().numpy()), bits(r.dot)) and np.array_equal(bits(jv.cpu().numpy()), bits(r.jv))
        assert np.array_equal(bits(nlp.hessian_vector_product(xt.detach(), dev(2.0 * fh), dev(2.0 * gh), ut).cpu().numpy()), bits(r.hv))


def test_torch_gradcheck(model):
    """torch.autograd.gradcheck in float64 with its default tolerances on one `default` pose, x perturbed on variables outside the base
    quaternion (two point coordinates and a force, the base position, joints, the com)"""
    import torch
    nlp, x, _ = _pose_nlp(model, "default", 1, 3000)
    idx = torch.tensor([0, 2, 5, 26, 48, 49, 50, 55, 60, 70, 77, 78, 79, 80], device="cuda")
    x0 = torch.tensor(x, device="cuda")
    z = x0[:, idx].clone().requires_grad_()

    def fn(zz):
        return nlp(x0.index_copy(1, idx, zz))
    assert torch.autograd.gradcheck(fn, (z,))


def test_a_stream_of_the_callers_gives_the_same_bits(model):
    import torch
    nlp, x, _ = _pose_nlp(model, "steps", 3, 3100)
    rng = np.random.RandomState(11)
    a, w, u = 0.9, dev(rng.standard_normal((3, nlp.m))), dev(rng.standard_normal((3, nlp.n)))

    def everything():
        xt = torch.tensor(x, device="cuda", requires_grad=True)
        f, g = nlp(xt)
        (gx,) = torch.autograd.grad((f ** 2).sum() + (w * g ** 2).sum(), xt, create_graph=True)
        (h,) = torch.autograd.grad((gx * u).sum(), xt)
        dot, jv = nlp.jacobian_vector_product(xt.detach(), u)
        return [f.detach(), g.detach(), gx.detach(), h, dot, jv, nlp.lagrangian_gradient(xt.detach(), a, w), nlp.hessian_vector_product(xt.detach(), a, w, u)]
    ref = [t.cpu() for t in everything()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = everything()
    side.synchronize()
    for q, (s, t) in enumerate(zip(got, ref)):
        assert torch.equal(s.cpu().view(torch.int64), t.view(torch.int64)), q


def test_torch_binding_refuses_wrong_tensors(model):
    import torch
    nlp, x, _ = _pose_nlp(model, "default", 2, 3200)
    good = torch.tensor(x, device="cuda")
    lam = torch.zeros((2, nlp.m), dtype=torch.float64, device="cuda")
    for exc, bad in ((TypeError, good.float()), (ValueError, good.cpu()), (ValueError, good[:1]), (ValueError, good.t().contiguous().t()), (TypeError, x)):
        with pytest.raises(exc):
            nlp(bad)
        with pytest.raises(exc):
            nlp.jacobian_vector_product(good, bad)
        with pytest.raises(exc):
            nlp.hessian_vector_product(good, 1.0, lam, bad)
    with pytest.raises(ValueError):
        nlp.lagrangian_gradient(good, 1.0, lam[:, :-1])
