"""GPU: the Hessian-vector product y = H(x, sigma, lambda) v in one launch (hipnlp_eval_hess_vec_device, hipnlp_knot_hvp_kernel), the
product from stored values (hipnlp_hess_times_device, hipnlp_hess_times_kernel) and the double backward of hippopt_amd.autograd built on
them.  Bounds: tests/hvp_check.py — against the oracle TOL sum_c s_ic |v_c| + 2 gamma_{K_i+1} S_i, against the handle's own
hipnlp_eval_hess_device values 2 gamma_{K_i+1} S_i; every figure is printed before it is asserted."""
import json
import os

import numpy as np
import pytest

from hippopt_amd.kinodyn_settings import periodic_step_settings, ramp_settings, stairs_settings
from hippopt_amd.synthetic import make_workload, place_on_step_flanks
from hvp_check import check, full_multipliers, oracle_bound, own_bound, rel, touch_counts
from test_gpu_lagrangian_grad import PLANNERS, lgrad, periodic_cost_ends_settings, sigma_cycle

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def hvp(eng, x, sigma, lam, v):
    """y [batch, n] of the fused launch from numpy inputs (a NaN-filled destination)"""
    import torch
    xd, sd, ld, vd = dev(x), dev(sigma), dev(lam), dev(v)
    out = torch.full((eng.batch, eng.n), float("nan"), dtype=torch.float64, device="cuda")
    eng.eval_hess_vec_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), vd.data_ptr(), out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def hess_values(eng, x, sigma, lam):
    """the value run [batch, nnz_h] of hipnlp_eval_hess_device, as a device tensor"""
    import torch
    xd, sd, ld = dev(x), dev(sigma), dev(lam)
    vals = torch.full((eng.batch, eng.hess_nnz()), float("nan"), dtype=torch.float64, device="cuda")
    eng.eval_hess_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), vals.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return vals


def hess_times(eng, vals, v):
    import torch
    vd = dev(v)
    out = torch.full((eng.batch, eng.n), float("nan"), dtype=torch.float64, device="cuda")
    eng.hess_times_device(vals.data_ptr(), vd.data_ptr(), out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def against_oracle(model, st, x, p, lifted, smooth, seed):
    from hippopt_amd.hipnlp import HipNlp
    from oracle_lib import Oracle
    B = x.shape[0]
    eng = HipNlp(st, model, batch=B, detect_simple_bounds=lifted)
    eng.set_params(p)
    rng = np.random.RandomState(seed)
    lam, v = rng.standard_normal((B, eng.m)), rng.standard_normal((B, eng.n))
    sigma = sigma_cycle(B, seed)
    y = hvp(eng, x, sigma, lam, v)
    assert np.all(np.isfinite(y))
    orc = Oracle(st, model)
    ir, jc = eng.hess_sparsity()
    k_i = touch_counts(ir, jc, eng.n)
    kept = eng.lift_map(with_bounds=False)[0]
    for b in range(B):
        iro, jco, valo = orc.hess(x[b], p[b], float(sigma[b]), full_multipliers(lam[b], kept))
        ref, bound = oracle_bound(iro, jco, valo, ir, jc, v[b], k_i, smooth)
        check(y[b], ref, bound, "N=%d B=%d lifted=%s b=%d sigma=%g" % (st.horizon_length, B, lifted, b, sigma[b]))


def stairs_200x16(model):
    N, B = 200, 16
    st = stairs_settings(N, model)
    base_x, base_p = make_workload(st, model, batch=1, seed=1005)
    x = np.repeat(base_x, B, axis=0)
    for b in range(B):
        x[b] += 0.02 * np.random.RandomState(2000 + b).standard_normal(x.shape[1])
    place_on_step_flanks(x[:2], st, seed=5)   # two guesses with contact points on the flanks of the bumps
    return st, x, np.repeat(base_p, B, axis=0)


@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("horizon", [2, 3, 30, 100])
@pytest.mark.parametrize("planner", list(PLANNERS))
def test_matches_oracle_on_the_planners(model, planner, horizon, lifted):
    st = PLANNERS[planner](horizon, model)
    seed = 6000 + horizon + 100 * list(PLANNERS).index(planner)
    x, p = make_workload(st, model, batch=3, seed=seed)
    against_oracle(model, st, x, p, lifted, False, seed)


@pytest.mark.parametrize("lifted", [False, True])
def test_matches_oracle_on_the_stairs_200x16(model, lifted):
    st, x, p = stairs_200x16(model)
    against_oracle(model, st, x, p, lifted, True, 87)


@pytest.mark.parametrize("lifted", [False, True])
def test_matches_oracle_on_the_ramp(model, lifted):
    st = ramp_settings(50, model)
    x, p = make_workload(st, model, batch=3, seed=4321)
    place_on_step_flanks(x[:1], st, seed=3)
    against_oracle(model, st, x, p, lifted, True, 88)


def problem(model, case):
    if case == "stairs_200x16":
        return stairs_200x16(model)
    if case == "cost_ends_30x4":
        st = periodic_cost_ends_settings(30, model)
        return (st,) + tuple(make_workload(st, model, batch=4, seed=6150))
    B = {"planar_100x64": 64, "planar_100x1": 1}[case]
    st = periodic_step_settings(100, model)
    return (st,) + tuple(make_workload(st, model, batch=B, seed=6100))


@pytest.mark.parametrize("case", ["planar_100x64", "stairs_200x16"])
def test_own_values_bound(model, case):
    from hippopt_amd.hipnlp import HipNlp
    st, x, p = problem(model, case)
    B = x.shape[0]
    eng = HipNlp(st, model, batch=B)
    eng.set_params(p)
    rng = np.random.RandomState(19)
    lam, v = rng.standard_normal((B, eng.m)), rng.standard_normal((B, eng.n))
    sigma = sigma_cycle(B, 19)
    y = hvp(eng, x, sigma, lam, v)
    vals = hess_values(eng, x, sigma, lam).cpu().numpy()
    ir, jc = eng.hess_sparsity()
    k_i = touch_counts(ir, jc, eng.n)
    for b in range(B):
        ref, bound = own_bound(ir, jc, vals[b], v[b], k_i)
        check(y[b], ref, bound, "%s own values b=%d" % (case, b))


@pytest.mark.parametrize("case", ["planar_100x64", "planar_100x1", "stairs_200x16", "cost_ends_30x4"])
def test_fused_equals_stored_values_bitwise(model, case):
    """(planar_100x1: the launch where hipnlp_eval_hess_device runs the FULL layout; cost_ends: the periodicity coupling on)"""
    from hippopt_amd.hipnlp import HipNlp
    st, x, p = problem(model, case)
    B = x.shape[0]
    eng = HipNlp(st, model, batch=B)
    eng.set_params(p)
    rng = np.random.RandomState(23)
    lam, v = rng.standard_normal((B, eng.m)), rng.standard_normal((B, eng.n))
    sigma = sigma_cycle(B, 23) + (0.25 if case == "cost_ends_30x4" else 0.0)   # (a coupling value of zero would hide the coupling term)
    y = hvp(eng, x, sigma, lam, v)
    z = hess_times(eng, hess_values(eng, x, sigma, lam), v)
    print("%s: %d of %d entries differ" % (case, int((bits(y) != bits(z)).sum()), y.size))
    assert np.all(np.isfinite(y)) and np.array_equal(bits(y), bits(z))
    if case == "cost_ends_30x4":   # the coupling term is really there: v at the other horizon end changes y at this end
        v2 = v.copy()
        v2[:, 189 * 29:189 * 30] += 1.0
        y2 = hvp(eng, x, sigma, lam, v2)
        assert np.any(y2[:, :189] != y[:, :189]) and np.array_equal(bits(y2[:, 189:189 * 29]), bits(y[:, 189:189 * 29]))


def test_batch_positions_and_jac_orders_give_the_same_bits(model):
    from hippopt_amd.hipnlp import HipNlp
    st = periodic_step_settings(100, model)
    B = 64
    x, p = make_workload(st, model, batch=B, seed=6300)
    ccs = HipNlp(st, model, batch=B)
    ccs.set_params(p)
    vf = HipNlp(st, model, batch=B, jac_varying_first=True)
    vf.set_params(p)
    rng = np.random.RandomState(4)
    lam, v = rng.standard_normal((B, ccs.m)), rng.standard_normal((B, ccs.n))
    sigma = sigma_cycle(B, 4)
    a, c = hvp(ccs, x, sigma, lam, v), hvp(vf, x, sigma, lam, v)
    assert np.array_equal(bits(a), bits(c))
    one = HipNlp(st, model, batch=1)
    for b in range(B):
        one.set_params(p[b:b + 1])
        s = hvp(one, x[b:b + 1], sigma[b:b + 1], lam[b:b + 1], v[b:b + 1])
        assert np.array_equal(bits(s[0]), bits(a[b])), b


@pytest.mark.parametrize("name", ["planner_periodic_N3", "planner_single_N3", "planner_costends_N2", "planner_stairs_N3", "planner_ramp_N3"])
def test_reference_planner_fixture(model, name):
    from hippopt_amd.hipnlp import HipNlp
    from test_golden_planner import GOLD, settings_for
    z = np.load(os.path.join(GOLD, name + ".npz"))
    eng = HipNlp(settings_for(json.loads(str(z["meta"])), model), model, batch=1)
    eng.set_params(z["p"][None, :])
    dirs, want = np.asarray(z["hess_dirs"]), np.asarray(z["hess_times_dirs"])
    dirs, want = (dirs, want) if dirs.shape[-1] == eng.n else (dirs.T, want.T)
    assert dirs.shape == (4, eng.n)
    sigma, lam = np.array([float(z["hess_sigma"])]), z["hess_lambda"][None, :]
    vals = hess_values(eng, z["x"][None, :], sigma, lam)
    for j in range(4):
        y = hvp(eng, z["x"][None, :], sigma, lam, dirs[j][None, :])[0]
        e = rel(y, want[j])
        print("%s direction %d: rel %.3e" % (name, j, e))
        assert e < (1e-9 if ("stairs" in name or "ramp" in name) else 1e-11)
        assert np.array_equal(bits(hess_times(eng, vals, dirs[j][None, :])[0]), bits(y))


def test_guard_words_around_the_destination(model):
    import torch
    from hippopt_amd.hipnlp import HipNlp
    B, G = 3, 256
    for st in (stairs_settings(7, model), periodic_cost_ends_settings(5, model)):
        x, p = make_workload(st, model, batch=B, seed=6400)
        eng = HipNlp(st, model, batch=B)
        eng.set_params(p)
        rng = np.random.RandomState(1)
        xd, sd, ld, vd = dev(x), dev(np.full(B, 1.1)), dev(rng.standard_normal((B, eng.m))), dev(rng.standard_normal((B, eng.n)))
        vals = hess_values(eng, x, np.full(B, 1.1), ld.cpu().numpy())
        stream = torch.cuda.current_stream().cuda_stream
        for fused in (True, False):
            buf = torch.full((B * eng.n + 2 * G,), float("nan"), dtype=torch.float64, device="cuda")
            buf[:G] = 1234.5
            buf[G + B * eng.n:] = 1234.5
            if fused:
                eng.eval_hess_vec_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), vd.data_ptr(), buf.data_ptr() + 8 * G, stream=stream)
            else:
                eng.hess_times_device(vals.data_ptr(), vd.data_ptr(), buf.data_ptr() + 8 * G, stream=stream)
            torch.cuda.synchronize()
            h = buf.cpu().numpy()
            assert np.all(h[:G] == 1234.5) and np.all(h[G + B * eng.n:] == 1234.5)
            body = h[G:G + B * eng.n].reshape(B, eng.n)
            assert np.all(np.isfinite(body))                                  # every entry overwritten
            assert np.array_equal(bits(body[:, -6:]), np.zeros((B, 6), np.int64))   # the horizon-global entries: +0.0


def test_error_codes(model):
    import torch
    from hippopt_amd.hipnlp import HipNlp, HipNlpError
    st = periodic_step_settings(6, model)
    x, p = make_workload(st, model, batch=1, seed=6500)
    xd = dev(x)
    sd = torch.ones(1, dtype=torch.float64, device="cuda")
    out = torch.zeros((1, x.shape[1]), dtype=torch.float64, device="cuda")
    plain = HipNlp(st, model)
    ld = torch.zeros((1, plain.m), dtype=torch.float64, device="cuda")
    vals = torch.zeros((1, plain.hess_nnz()), dtype=torch.float64, device="cuda")
    args = (xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), xd.data_ptr(), out.data_ptr())
    with pytest.raises(HipNlpError) as e:
        plain.eval_hess_vec_device(*args)          # parameters not set
    assert e.value.code == -4                      # HIPNLP_E_PARAMS
    plain.hess_times_device(vals.data_ptr(), xd.data_ptr(), out.data_ptr())   # (needs no parameters)
    torch.cuda.synchronize()
    front = HipNlp(st, model, devices=[0, 0])      # a two-shard front of device 0
    front.set_params(p)
    shard = HipNlp(st, model, knot_begin=0, knot_end=3)
    shard.set_params(p)
    for eng, word in ((front, "multi-device"), (shard, "shard")):
        with pytest.raises(HipNlpError) as e:
            eng.eval_hess_vec_device(*args)
        assert e.value.code == -6 and word in str(e.value)
        with pytest.raises(HipNlpError) as e:
            eng.hess_times_device(vals.data_ptr(), xd.data_ptr(), out.data_ptr())
        assert e.value.code == -6 and word in str(e.value)


def test_other_launches_of_the_handle_are_undisturbed(model):
    from hippopt_amd.hipnlp import HipNlp
    st = periodic_cost_ends_settings(30, model)
    B = 4
    x, p = make_workload(st, model, batch=B, seed=6600)
    eng = HipNlp(st, model, batch=B)
    eng.set_params(p)
    rng = np.random.RandomState(6)
    lam, v = rng.standard_normal((B, eng.m)), rng.standard_normal((B, eng.n))
    sigma = sigma_cycle(B, 6) + 0.5

    def others():
        h = hess_values(eng, x, sigma, lam).cpu().numpy()
        hh = eng.eval_hess(x, sigma, lam)
        ev = eng.eval(x)
        lg = lgrad(eng, x, sigma, lam)
        return [h, hh, lg] + [np.asarray(o) for o in ev]
    before = others()
    y = hvp(eng, x, sigma, lam, v)
    after = others()
    for a, c in zip(before, after):
        assert np.array_equal(bits(a), bits(c))
    assert np.array_equal(bits(hvp(eng, x, sigma, lam, v)), bits(y))


def test_torch_second_derivatives(model):
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    st = periodic_step_settings(30, model)
    B = 8
    x, p = make_workload(st, model, batch=B, seed=6700)
    rng = np.random.RandomState(12)
    for lifted in (False, True):
        nlp = KinodynamicNLP(st, model, batch=B, detect_simple_bounds=lifted)
        nlp.set_params(p)
        a = 0.37
        w, u = dev(rng.standard_normal((B, nlp.m))), dev(rng.standard_normal((B, nlp.n)))
        xt = torch.tensor(x, device="cuda", requires_grad=True)
        sd = torch.full((B,), a, dtype=torch.float64, device="cuda")
        # the method is the raw launch
        hv = nlp.hessian_vector_product(xt.detach(), a, w, u)
        raw = hvp(nlp.engine, x, sd.cpu().numpy(), w.cpu().numpy(), u.cpu().numpy())
        assert np.array_equal(bits(hv.cpu().numpy()), bits(raw))
        assert torch.equal(nlp.hessian_vector_product(xt.detach(), sd, w, u).view(torch.int64), hv.view(torch.int64))
        # stored values
        H = nlp.hessian(xt.detach(), a, w)
        assert H.values.shape == (B, nlp.engine.hess_nnz())
        assert torch.equal(H.matvec(u).view(torch.int64), hv.view(torch.int64))
        # d/dx of (lagrangian gradient . u)
        lg = nlp.lagrangian_gradient(xt, a, w)
        assert lg.requires_grad and torch.equal(lg.detach().view(torch.int64), nlp.lagrangian_gradient(xt.detach(), a, w).view(torch.int64))
        (h1,) = torch.autograd.grad((lg * u).sum(), xt)
        assert torch.equal(h1.view(torch.int64), hv.view(torch.int64))
        # double backward through nlp(x), a loss linear in f and g
        f, g = nlp(xt)
        (gx,) = torch.autograd.grad(a * f.sum() + (w * g).sum(), xt, create_graph=True)
        assert gx.requires_grad
        f1, g1 = nlp(xt)
        (gx1,) = torch.autograd.grad(a * f1.sum() + (w * g1).sum(), xt)          # the first-order path: the parent's launch
        assert not gx1.requires_grad
        assert torch.equal(gx.detach().view(torch.int64), gx1.view(torch.int64))
        assert torch.equal(gx1.view(torch.int64), nlp.lagrangian_gradient(xt.detach(), a, w).view(torch.int64))
        (h2,) = torch.autograd.grad((gx * u).sum(), xt)
        assert torch.equal(h2.view(torch.int64), hv.view(torch.int64))
        # a loss that is not linear in f: the double backward needs grad f . w, which the engine does not have
        f, g = nlp(xt)
        (gq,) = torch.autograd.grad((f ** 2).sum(), xt, create_graph=True)
        with pytest.raises(NotImplementedError):
            torch.autograd.grad((gq * u).sum(), xt)
        f, g = nlp(xt)
        (gq,) = torch.autograd.grad((g ** 2).sum(), xt, create_graph=True)
        with pytest.raises(NotImplementedError):
            torch.autograd.grad((gq * u).sum(), xt)
    # on a stream of the caller's: the same bits, ordered on that stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xs = torch.tensor(x, device="cuda", requires_grad=True)
        fs, gs = nlp(xs)
        (gxs,) = torch.autograd.grad(a * fs.sum() + (w * gs).sum(), xs, create_graph=True)
        (h3,) = torch.autograd.grad((gxs * u).sum(), xs)
        same = (torch.equal(h3.view(torch.int64), hv.view(torch.int64))
                and torch.equal(nlp.hessian_vector_product(xs.detach(), a, w, u).view(torch.int64), hv.view(torch.int64))
                and torch.equal(nlp.hessian(xs.detach(), a, w).matvec(u).view(torch.int64), hv.view(torch.int64)))
    side.synchronize()
    assert same


def test_torch_binding_refuses_wrong_tensors(model):
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    st = periodic_step_settings(4, model)
    B = 2
    x, p = make_workload(st, model, batch=B, seed=6800)
    nlp = KinodynamicNLP(st, model, batch=B)
    nlp.set_params(p)
    good = torch.tensor(x, device="cuda")
    lam = torch.zeros((B, nlp.m), dtype=torch.float64, device="cuda")
    wide = torch.zeros((B, 2 * nlp.n), dtype=torch.float64, device="cuda")
    bad = {"dtype": (TypeError, good.float()), "device": (ValueError, good.cpu()), "shape": (ValueError, good[:1]),
           "columns": (ValueError, torch.zeros((B, nlp.n + 1), dtype=torch.float64, device="cuda")), "strided": (ValueError, wide[:, ::2])}
    H = nlp.hessian(good, 1.0, lam)
    for name, (exc, t) in bad.items():
        with pytest.raises(exc):
            nlp.hessian_vector_product(t, 1.0, lam, good)
        with pytest.raises(exc):
            nlp.hessian_vector_product(good, 1.0, lam, t)
        with pytest.raises(exc):
            nlp.hessian(t, 1.0, lam)
        with pytest.raises(exc):
            H.matvec(t)
    with pytest.raises(TypeError):
        nlp.hessian_vector_product(good, 1.0, lam.float(), good)
    with pytest.raises(ValueError):
        nlp.hessian_vector_product(good, 1.0, lam[:, :-1], good)
    with pytest.raises(ValueError):
        nlp.hessian_vector_product(good, torch.ones(B + 1, dtype=torch.float64, device="cuda"), lam, good)
    with pytest.raises(TypeError):
        nlp.hessian_vector_product(good, 1.0, lam, np.zeros((B, nlp.n)))
    assert torch.all(torch.isfinite(nlp.hessian_vector_product(good, 1.0, lam, good)))
