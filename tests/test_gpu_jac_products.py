"""GPU: the products with a stored value run of jac g — J v and grad f . v (hipnlp_jac_times_device) and sigma grad f + J^T lambda
(hipnlp_jac_transpose_times_device) — and what hippopt_amd.autograd builds on them.  Unit vectors through the batch dimension give the
columns and rows of the handle's own hipnlp_eval_device run bit for bit; the device equals the CPU emulation (tests/jprod_emu) bit for
bit; against the oracle the bounds are those of pose_products_check.check_first_order with n variables (TOL 1e-11 planar, 1e-9 smooth,
as lgrad_check); every figure is printed before it is asserted."""
import numpy as np
import pytest

import hvp_check
import lgrad_check
from hippopt_amd.kinodyn_settings import periodic_step_settings, ramp_settings, stairs_settings
from hippopt_amd.synthetic import make_workload, place_on_step_flanks
from lgrad_check import TOL_PLANAR, TOL_SMOOTH, check, column_counts, full_multipliers, gamma, oracle_bound, own_bound
from pose_products_check import row_times
from test_gpu_lagrangian_grad import PLANNERS, lgrad, sigma_cycle

pytestmark = pytest.mark.gpu
NXK = 189


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def nans(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def value_run(eng, x):
    """(grad f, jac g) device tensors [batch, .] of the handle's own hipnlp_eval_device"""
    import torch
    xd = dev(x)
    grad, jac = nans(eng.batch, eng.n), nans(eng.batch, eng.nnz)
    eng.eval_device(xd.data_ptr(), 0, grad.data_ptr(), 0, jac.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(jac).all()) and bool(torch.isfinite(grad).all())
    return grad, jac


def jac_times(eng, jac, v, grad=None, want_jv=True):
    """(J v [batch, m] or None, grad f . v [batch] or None) as numpy, NaN-filled destinations"""
    import torch
    vd = dev(v)
    jv = nans(eng.batch, eng.m) if want_jv else None
    dot = nans(eng.batch) if grad is not None else None
    eng.jac_times_device(jac.data_ptr(), vd.data_ptr(), jv.data_ptr() if want_jv else 0, dot.data_ptr() if grad is not None else 0,
                         grad_values_ptr=grad.data_ptr() if grad is not None else 0, stream=stream())
    torch.cuda.synchronize()
    return (jv.cpu().numpy() if want_jv else None), (dot.cpu().numpy() if grad is not None else None)


def jac_transpose_times(eng, jac, lam, grad=None, sigma=None):
    import torch
    ld, out = dev(lam), nans(eng.batch, eng.n)
    sd = dev(sigma) if sigma is not None else None
    eng.jac_transpose_times_device(jac.data_ptr(), ld.data_ptr(), out.data_ptr(), grad_values_ptr=grad.data_ptr() if grad is not None else 0,
                                   obj_factor_ptr=sd.data_ptr() if sd is not None else 0, stream=stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- unit vectors through the batch dimension ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("vary_first", [False, True])
@pytest.mark.parametrize("horizon", [2, 3, 4])
@pytest.mark.parametrize("planner", ["periodic", "single"])
def test_unit_vectors_give_the_columns_and_rows_of_the_own_run(model, planner, horizon, vary_first, lifted):
    from hippopt_amd.hipnlp import HipNlp
    st = PLANNERS[planner](horizon, model)
    x1, p1 = make_workload(st, model, batch=1, seed=7100 + horizon)
    probe = HipNlp(st, model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
    n, m = probe.n, probe.m
    ir, jc = probe.sparsity()
    e = np.arange(probe.nnz)
    # batch = n: trajectory c multiplies by e_c
    eng = HipNlp(st, model, batch=n, detect_simple_bounds=lifted, jac_varying_first=vary_first)
    eng.set_params(np.repeat(p1, n, axis=0))
    grad, jac = value_run(eng, np.repeat(x1, n, axis=0))
    jv, dot = jac_times(eng, jac, np.eye(n), grad=grad)
    jh, gh = jac.cpu().numpy(), grad.cpu().numpy()
    want = np.zeros((n, m))
    want[jc, ir] = jh[jc, e]
    assert np.array_equal(bits(jv), bits(want)), np.argwhere(bits(jv) != bits(want))[:4]
    assert np.array_equal(bits(dot), bits(gh[np.arange(n), np.arange(n)] + 0.0))   # (one product, the rest +0.0)
    # batch = m: trajectory i multiplies by e_i from the left
    eng = HipNlp(st, model, batch=m, detect_simple_bounds=lifted, jac_varying_first=vary_first)
    eng.set_params(np.repeat(p1, m, axis=0))
    grad, jac = value_run(eng, np.repeat(x1, m, axis=0))
    out = jac_transpose_times(eng, jac, np.eye(m))
    jh = jac.cpu().numpy()
    want = np.zeros((m, n))
    want[ir, jc] = jh[ir, e]
    assert np.array_equal(bits(out), bits(want)), np.argwhere(bits(out) != bits(want))[:4]


# ---- device == emulation, bit for bit ---------------------------------------------------------------------------------------------------
EMU_CASES = [("periodic", 2, False), ("periodic", 3, False), ("periodic", 4, True), ("periodic", 30, False), ("periodic", 30, True), ("single", 3, False),
             ("cost_ends", 4, False), ("stairs", 7, False), ("stairs", 7, True)]


@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("name,horizon,vary_first", EMU_CASES)
def test_device_equals_the_emulation_bitwise(model, name, horizon, vary_first, lifted):
    from hippopt_amd.hipnlp import HipNlp
    from jprod_emu_lib import JprodEmu
    st = stairs_settings(horizon, model) if name == "stairs" else PLANNERS[name](horizon, model)
    B = 3
    x, p = make_workload(st, model, batch=B, seed=7200 + horizon)
    eng = HipNlp(st, model, batch=B, detect_simple_bounds=lifted, jac_varying_first=vary_first)
    eng.set_params(p)
    emu = JprodEmu(st, model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
    assert (emu.n, emu.m, emu.nnz) == (eng.n, eng.m, eng.nnz)
    rng = np.random.RandomState(horizon)
    v, lam, sigma = rng.standard_normal((B, eng.n)), rng.standard_normal((B, eng.m)), sigma_cycle(B, 3) + 0.25
    grad, jac = value_run(eng, x)
    jv, dot = jac_times(eng, jac, v, grad=grad)
    out = jac_transpose_times(eng, jac, lam, grad=grad, sigma=sigma)
    out0 = jac_transpose_times(eng, jac, lam)
    gh, jh = grad.cpu().numpy(), jac.cpu().numpy()
    for b in range(B):
        ejv, edot, _, _ = emu.jac_times(jh[b], v[b], grad=gh[b])
        assert np.array_equal(bits(jv[b]), bits(ejv)), ("J v", b, np.flatnonzero(bits(jv[b]) != bits(ejv))[:6])
        assert bits([dot[b]])[0] == bits([edot])[0], ("grad f . v", b, dot[b], edot)
        eout, _ = emu.jac_transpose_times(jh[b], lam[b], sigma=sigma[b], grad=gh[b])
        assert np.array_equal(bits(out[b]), bits(eout)), ("xbar", b)
        eout, _ = emu.jac_transpose_times(jh[b], lam[b])
        assert np.array_equal(bits(out0[b]), bits(eout)), ("J^T lam", b)


# ---- against the oracle -------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_outputs(model, key, st, x, p):
    """(irow, jcol, [grad f, jac g per trajectory]) of the oracle, computed once per case"""
    from oracle_lib import Oracle
    if key not in _ORACLE:
        orc = Oracle(st, model)
        _ORACLE[key] = orc.sparsity() + ([orc.eval(x[b], p[b]) for b in range(x.shape[0])],)
    return _ORACLE[key]


def against_oracle(model, key, st, x, p, lifted, tol, seed):
    from hippopt_amd.hipnlp import HipNlp
    B = x.shape[0]
    eng = HipNlp(st, model, batch=B, detect_simple_bounds=lifted)
    eng.set_params(p)
    n, m = eng.n, eng.m
    rng = np.random.RandomState(seed)
    v, lam, sigma = rng.standard_normal((B, n)), rng.standard_normal((B, m)), sigma_cycle(B, seed)
    grad, jac = value_run(eng, x)
    jv, dot = jac_times(eng, jac, v, grad=grad)
    xbar = jac_transpose_times(eng, jac, lam, grad=grad, sigma=sigma)
    fused = lgrad(eng, x, sigma, lam)
    gh, jh = grad.cpu().numpy(), jac.cpu().numpy()
    ir, jc = eng.sparsity()
    iro, jco, outs = oracle_outputs(model, key, st, x, p)
    kept = eng.lift_map(with_bounds=False)[0]
    k_c, k_i = column_counts(jc, n), np.bincount(ir, minlength=m)
    g2, gd = 2.0 * gamma(k_i + 1), 2.0 * float(gamma(n + 1))
    sel = kept >= 0
    for b in range(B):
        what = "%s lifted=%s b=%d" % (key, lifted, b)
        _, grado, _, jaco = outs[b]
        grado, jaco = np.asarray(grado), np.asarray(jaco)
        # xbar
        ref, bound = own_bound(gh[b], ir, jc, jh[b], sigma[b], lam[b])
        check(xbar[b], ref, bound, what + ": xbar against the own run")
        err = np.abs(xbar[b] - fused[b])
        print("%s: xbar against the fused launch: max %.3e, worst ratio %.3e" % (what, err.max(), np.max(err / np.where(bound > 0, bound, 1.0))))
        assert np.all(err <= bound)
        ref, bound = oracle_bound(grado, iro, jco, jaco, sigma[b], full_multipliers(lam[b], kept), k_c, tol)
        check(xbar[b], ref, bound, what + ": xbar against the oracle")
        # J v
        check(jv[b], row_times(ir, jc, jh[b], v[b], m), g2 * row_times(ir, jc, jh[b], v[b], m, absolute=True), what + ": J v against the own run")
        mf = kept.size
        ref = row_times(iro, jco, jaco, v[b], mf)
        bound = tol * row_times(iro, jco, jaco, v[b], mf, floor=True) + 2.0 * gamma(np.bincount(iro, minlength=mf) + 1) * row_times(iro, jco, jaco, v[b], mf, absolute=True)
        check(jv[b][kept[sel]], ref[sel], bound[sel], what + ": J v against the oracle")
        # grad f . v
        for src, t, label in ((gh[b], 0.0, "the own run"), (grado, tol, "the oracle")):
            ref = np.array([np.dot(src, v[b])])
            bound = np.array([t * np.dot(np.maximum(1.0, np.abs(src)), np.abs(v[b])) + gd * np.dot(np.abs(src), np.abs(v[b]))])
            check(np.atleast_1d(dot[b]), ref, bound, what + ": grad f . v against " + label)


@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("horizon", [2, 3, 30])
@pytest.mark.parametrize("planner", list(PLANNERS))
def test_matches_oracle_on_the_planners(model, planner, horizon, lifted):
    st = PLANNERS[planner](horizon, model)
    seed = 7300 + horizon + 100 * list(PLANNERS).index(planner)
    x, p = make_workload(st, model, batch=3, seed=seed)
    against_oracle(model, "%s N=%d" % (planner, horizon), st, x, p, lifted, TOL_PLANAR, seed)


@pytest.mark.parametrize("lifted", [False, True])
def test_matches_oracle_on_the_ramp(model, lifted):
    st = ramp_settings(50, model)
    x, p = make_workload(st, model, batch=3, seed=7321)
    place_on_step_flanks(x[:1], st, seed=3)
    against_oracle(model, "ramp N=50", st, x, p, lifted, TOL_SMOOTH, 79)


# ---- memory and arguments ----------------------------------------------------------------------------------------------------------------
def test_guard_words_and_missing_destinations(model):
    import torch
    from hippopt_amd.hipnlp import HipNlp
    B, G = 3, 256
    for st in (stairs_settings(7, model), PLANNERS["periodic"](3, model), PLANNERS["single"](2, model)):
        x, p = make_workload(st, model, batch=B, seed=7400)
        eng = HipNlp(st, model, batch=B)
        eng.set_params(p)
        rng = np.random.RandomState(1)
        grad, jac = value_run(eng, x)
        vd, ld, sd = dev(rng.standard_normal((B, eng.n))), dev(rng.standard_normal((B, eng.m))), dev(np.full(B, 1.1))

        def guarded(words):
            buf = torch.full((words + 2 * G,), float("nan"), dtype=torch.float64, device="cuda")
            buf[:G] = 1234.5
            buf[G + words:] = 1234.5
            return buf

        def body(buf, words):
            h = buf.cpu().numpy()
            assert np.all(h[:G] == 1234.5) and np.all(h[G + words:] == 1234.5)
            assert np.all(np.isfinite(h[G:G + words]))   # every entry overwritten
            return h[G:G + words]
        jv, dot, out = guarded(B * eng.m), guarded(B), guarded(B * eng.n)
        eng.jac_times_device(jac.data_ptr(), vd.data_ptr(), jv.data_ptr() + 8 * G, dot.data_ptr() + 8 * G, grad_values_ptr=grad.data_ptr(), stream=stream())
        eng.jac_transpose_times_device(jac.data_ptr(), ld.data_ptr(), out.data_ptr() + 8 * G, grad_values_ptr=grad.data_ptr(), obj_factor_ptr=sd.data_ptr(), stream=stream())
        torch.cuda.synchronize()
        jv_both, dot_both = body(jv, B * eng.m).copy(), body(dot, B).copy()
        body(out, B * eng.n)
        # one destination at a time: the same bits, nothing else written
        jv1, dot1 = guarded(B * eng.m), guarded(B)
        eng.jac_times_device(jac.data_ptr(), vd.data_ptr(), jv1.data_ptr() + 8 * G, 0, stream=stream())
        eng.jac_times_device(jac.data_ptr(), vd.data_ptr(), 0, dot1.data_ptr() + 8 * G, grad_values_ptr=grad.data_ptr(), stream=stream())
        torch.cuda.synchronize()
        assert np.array_equal(bits(body(jv1, B * eng.m)), bits(jv_both)) and np.array_equal(bits(body(dot1, B)), bits(dot_both))


def test_batch_positions_give_the_same_bits(model):
    from hippopt_amd.hipnlp import HipNlp
    st = PLANNERS["periodic"](5, model)
    B = 8
    x, p = make_workload(st, model, batch=B, seed=7500)
    eng = HipNlp(st, model, batch=B)
    eng.set_params(p)
    rng = np.random.RandomState(4)
    v, lam, sigma = rng.standard_normal((B, eng.n)), rng.standard_normal((B, eng.m)), rng.uniform(0.2, 2.0, B)
    grad, jac = value_run(eng, x)
    jv, dot = jac_times(eng, jac, v, grad=grad)
    out = jac_transpose_times(eng, jac, lam, grad=grad, sigma=sigma)
    for b in range(B):
        one = HipNlp(st, model, batch=1)
        one.set_params(p[b:b + 1])
        g1, j1 = value_run(one, x[b:b + 1])
        assert np.array_equal(bits(j1.cpu().numpy()[0]), bits(jac.cpu().numpy()[b]))
        jv1, dot1 = jac_times(one, j1, v[b:b + 1], grad=g1)
        out1 = jac_transpose_times(one, j1, lam[b:b + 1], grad=g1, sigma=sigma[b:b + 1])
        assert np.array_equal(bits(jv1[0]), bits(jv[b])) and np.array_equal(bits(dot1), bits(dot[b:b + 1])) and np.array_equal(bits(out1[0]), bits(out[b]))


def test_error_codes(model):
    import torch
    from hippopt_amd.hipnlp import HipNlp, HipNlpError
    st = periodic_step_settings(6, model)
    x, p = make_workload(st, model, batch=1, seed=7600)
    plain = HipNlp(st, model)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    jac, grad, v, lam, jv, dot, out, sig = z(1, plain.nnz), z(1, plain.n), z(1, plain.n), z(1, plain.m), z(1, plain.m), z(1), z(1, plain.n), z(1)
    P = lambda t: t.data_ptr()  # noqa: E731
    plain.jac_times_device(P(jac), P(v), P(jv), P(dot), grad_values_ptr=P(grad))          # (needs no parameters)
    plain.jac_transpose_times_device(P(jac), P(lam), P(out))
    torch.cuda.synchronize()
    for call in (lambda: plain.jac_times_device(0, P(v), P(jv)), lambda: plain.jac_times_device(P(jac), 0, P(jv)),
                 lambda: plain.jac_times_device(P(jac), P(v), 0, 0, grad_values_ptr=P(grad)),            # both outputs missing
                 lambda: plain.jac_times_device(P(jac), P(v), P(jv), P(dot)),                            # dot without grad
                 lambda: plain.jac_transpose_times_device(0, P(lam), P(out)), lambda: plain.jac_transpose_times_device(P(jac), 0, P(out)),
                 lambda: plain.jac_transpose_times_device(P(jac), P(lam), 0),
                 lambda: plain.jac_transpose_times_device(P(jac), P(lam), P(out), grad_values_ptr=P(grad))):   # grad without obj_factor
        with pytest.raises(HipNlpError) as e:
            call()
        assert e.value.code == -1                   # HIPNLP_E_INVALID
    front = HipNlp(st, model, devices=[0, 0])       # a two-shard front of device 0
    front.set_params(p)
    shard = HipNlp(st, model, knot_begin=0, knot_end=3)
    shard.set_params(p)
    for eng, word in ((front, "multi-device"), (shard, "shard")):
        with pytest.raises(HipNlpError) as e:
            eng.jac_times_device(P(jac), P(v), P(jv))
        assert e.value.code == -6 and word in str(e.value)
        with pytest.raises(HipNlpError) as e:
            eng.jac_transpose_times_device(P(jac), P(lam), P(out))
        assert e.value.code == -6 and word in str(e.value)


# ---- autograd --------------------------------------------------------------------------------------------------------------------------------
def test_torch_jacobian_products_and_double_backward(model):
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    st = periodic_step_settings(30, model)
    B = 8
    x, p = make_workload(st, model, batch=B, seed=7700)
    rng = np.random.RandomState(12)
    eq = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))  # noqa: E731
    for lifted in (False, True):
        nlp = KinodynamicNLP(st, model, batch=B, detect_simple_bounds=lifted, jacobian_products=True)
        nlp.set_params(p)
        u, lam = dev(rng.standard_normal((B, nlp.n))), dev(rng.standard_normal((B, nlp.m)))
        xd = dev(x)
        J = nlp.jacobian(xd)
        assert J.values.shape == (B, nlp.engine.nnz) and J.grad.shape == (B, nlp.n)
        dot, jv = nlp.jacobian_vector_product(xd, u)
        d2, j2 = J.jvp(u)
        assert eq(dot, d2) and eq(jv, j2) and eq(J.matvec(u), jv) and eq(J.grad_dot(u), dot)
        raw_jv, raw_dot = jac_times(nlp.engine, J.values, u.cpu().numpy(), grad=J.grad)
        assert np.array_equal(bits(raw_jv), bits(jv.cpu().numpy())) and np.array_equal(bits(raw_dot), bits(dot.cpu().numpy()))
        ir, jc = nlp.engine.sparsity()
        r = J.rmatvec(0.37, lam).cpu().numpy()
        fused = nlp.lagrangian_gradient(xd, 0.37, lam).cpu().numpy()
        for b in range(B):
            _, bound = own_bound(J.grad[b].cpu().numpy(), ir, jc, J.values[b].cpu().numpy(), 0.37, lam[b].cpu().numpy())
            assert np.all(np.abs(r[b] - fused[b]) <= bound)
        # L = sum f^2 + sum g^2:  d/dx (grad L . u) = H(x, 2 f, 2 g) u + 2 (grad f . u) grad f + 2 J^T (J u)
        xt = torch.tensor(x, device="cuda", requires_grad=True)
        f, g = nlp(xt)
        (gL,) = torch.autograd.grad((f ** 2).sum() + (g ** 2).sum(), xt, create_graph=True)
        (got,) = torch.autograd.grad((gL * u).sum(), xt)
        fd, gd = f.detach(), g.detach()
        hv = nlp.hessian_vector_product(xd, (2.0 * fd).contiguous(), (2.0 * gd).contiguous(), u)
        first = nlp.lagrangian_gradient(xd, (2.0 * dot).contiguous(), (2.0 * jv).contiguous())
        want = (hv + first).cpu().numpy()
        hr, hc = nlp.engine.hess_sparsity()
        k_i = hvp_check.touch_counts(hr, hc, nlp.n)
        H = nlp.hessian(xd, (2.0 * fd).contiguous(), (2.0 * gd).contiguous()).values.cpu().numpy()
        got = got.cpu().numpy()
        for b in range(B):
            _, b_h = hvp_check.own_bound(hr, hc, H[b], u[b].cpu().numpy(), k_i)
            _, b_l = own_bound(J.grad[b].cpu().numpy(), ir, jc, J.values[b].cpu().numpy(), float(2.0 * dot[b]), (2.0 * jv[b]).cpu().numpy())
            check(got[b], want[b], b_h + b_l, "double backward lifted=%s b=%d" % (lifted, b))
        # a sigma / lam that requires grad gets grad f . w / J w
        sg = torch.full((B,), 0.8, dtype=torch.float64, device="cuda", requires_grad=True)
        lg = lam.clone().requires_grad_(True)
        out = nlp.lagrangian_gradient(xd, sg, lg)
        assert out.requires_grad
        gs, gl = torch.autograd.grad((out * u).sum(), (sg, lg))
        assert eq(gs, dot) and eq(gl, jv)
    # on a stream of the caller's: the same bits, ordered on that stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xs = dev(x)
        ds, js = nlp.jacobian_vector_product(xs, u)
        Js = nlp.jacobian(xs)
        same = eq(ds, dot) and eq(js, jv) and eq(Js.matvec(u), jv) and eq(Js.rmatvec(0.37, lam), J.rmatvec(0.37, lam))
    side.synchronize()
    assert same


def test_torch_binding_refuses_wrong_tensors(model):
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    st = periodic_step_settings(4, model)
    B = 2
    x, p = make_workload(st, model, batch=B, seed=7800)
    nlp = KinodynamicNLP(st, model, batch=B)
    assert nlp.jacobian_products is False
    nlp.set_params(p)
    good = torch.tensor(x, device="cuda")
    lam = torch.zeros((B, nlp.m), dtype=torch.float64, device="cuda")
    wide = torch.zeros((B, 2 * nlp.n), dtype=torch.float64, device="cuda")
    bad = {"dtype": (TypeError, good.float()), "device": (ValueError, good.cpu()), "shape": (ValueError, good[:1]),
           "columns": (ValueError, torch.zeros((B, nlp.n + 1), dtype=torch.float64, device="cuda")), "strided": (ValueError, wide[:, ::2])}
    J = nlp.jacobian(good)
    for name, (exc, t) in bad.items():
        for call in (lambda: nlp.jacobian(t), lambda: nlp.jacobian_vector_product(t, good), lambda: nlp.jacobian_vector_product(good, t),
                     lambda: J.matvec(t), lambda: J.grad_dot(t), lambda: J.jvp(t)):
            with pytest.raises(exc):
                call()
    for exc, t in ((TypeError, lam.float()), (ValueError, lam.cpu()), (ValueError, lam[:1]), (ValueError, lam[:, :-1])):
        with pytest.raises(exc):
            J.rmatvec(1.0, t)
    with pytest.raises(ValueError):
        J.rmatvec(torch.ones(B + 1, dtype=torch.float64, device="cuda"), lam)
