"""GPU: the KKT operator  top = (H + diag dx) v + J^T w,  bottom = J v - diag(dc) w  from stored value runs in ONE launch
(hipnlp_kkt_times_device, hipnlp_kkt_times_kernel) and hippopt_amd.autograd.KKTValues on it.  The device equals the CPU emulation
(tests/kkt_emu) bit for bit; without diagonals it is bit for bit hipnlp_hess_times_device + hipnlp_jac_transpose_times_device (one torch
addition) and hipnlp_jac_times_device, with diagonals the exactly rounded fused multiply-add of those; against the oracle the bound is the
sum of the bounds of the three parts (hvp_check.oracle_bound, lgrad_check.oracle_bound without a gradient, the J v bound of
tests/test_gpu_jac_products.py) plus 2^-52 |d v| for the diagonal term; every figure is printed before it is asserted."""
import numpy as np
import pytest

import hvp_check
import kkt_check
import lgrad_check
from hippopt_amd.kinodyn_settings import periodic_step_settings, ramp_settings, stairs_settings
from hippopt_amd.synthetic import make_workload, place_on_step_flanks
from kkt_check import bits
from lgrad_check import TOL_PLANAR, TOL_SMOOTH, gamma
from pose_products_check import row_times
from test_gpu_lagrangian_grad import PLANNERS

pytestmark = pytest.mark.gpu
MAKERS = dict(PLANNERS, stairs=stairs_settings, ramp=ramp_settings)
SMOOTH = ("stairs", "ramp")


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def nans(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Problem:
    """a handle with its two value runs at a seeded x, sigma, lambda, and seeded v, w, dx > 0, dc > 0 (numpy and device)"""

    def __init__(self, model, name, horizon, batch=2, lifted=False, vary_first=False, seed=0, same=False):
        import torch
        from hippopt_amd.hipnlp import HipNlp
        self.st = MAKERS[name](horizon, model)
        x, p = make_workload(self.st, model, batch=1 if same else batch, seed=8100 + seed)
        if name in SMOOTH:
            place_on_step_flanks(x[:1], self.st, seed=3)
        if same:
            x, p = np.repeat(x, batch, axis=0), np.repeat(p, batch, axis=0)
        self.x, self.p, self.B = x, p, batch
        self.eng = eng = HipNlp(self.st, model, batch=batch, detect_simple_bounds=lifted, jac_varying_first=vary_first)
        eng.set_params(p)
        rng = np.random.RandomState(seed)
        rows = 1 if same else batch
        rep = (lambda a: np.repeat(a, batch, axis=0)) if same else (lambda a: a)
        self.sigma = rep(rng.uniform(0.2, 2.0, rows))
        self.lam, self.v, self.w = rep(rng.standard_normal((rows, eng.m))), rep(rng.standard_normal((rows, eng.n))), rep(rng.standard_normal((rows, eng.m)))
        self.dx, self.dc = rep(rng.uniform(0.1, 3.0, (rows, eng.n))), rep(rng.uniform(0.1, 3.0, (rows, eng.m)))
        xd = dev(x)
        self.jac, self.hess = nans(batch, eng.nnz), nans(batch, eng.hess_nnz())
        eng.eval_device(xd.data_ptr(), 0, 0, 0, self.jac.data_ptr(), stream=stream())
        sd, ld = dev(self.sigma), dev(self.lam)
        eng.eval_hess_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), self.hess.data_ptr(), stream=stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(self.jac).all()) and bool(torch.isfinite(self.hess).all())
        self.vd, self.wd, self.dxd, self.dcd = dev(self.v), dev(self.w), dev(self.dx), dev(self.dc)

    def kkt(self, dx=False, dc=False):
        """(top [B, n], bottom [B, m]) of one launch into NaN-filled destinations, as numpy"""
        import torch
        eng = self.eng
        top, bottom = nans(self.B, eng.n), nans(self.B, eng.m)
        eng.kkt_times_device(self.hess.data_ptr(), self.jac.data_ptr(), self.vd.data_ptr(), self.wd.data_ptr(), top.data_ptr(), bottom.data_ptr(),
                             dx_ptr=self.dxd.data_ptr() if dx else 0, dc_ptr=self.dcd.data_ptr() if dc else 0, stream=stream())
        torch.cuda.synchronize()
        return top.cpu().numpy(), bottom.cpu().numpy()

    def three_launches(self):
        """(H v + J^T w [B, n] added by torch, J v [B, m]) through the three entry points the operator replaces"""
        import torch
        eng = self.eng
        hv, jt, jv = nans(self.B, eng.n), nans(self.B, eng.n), nans(self.B, eng.m)
        eng.hess_times_device(self.hess.data_ptr(), self.vd.data_ptr(), hv.data_ptr(), stream=stream())
        eng.jac_transpose_times_device(self.jac.data_ptr(), self.wd.data_ptr(), jt.data_ptr(), stream=stream())
        eng.jac_times_device(self.jac.data_ptr(), self.vd.data_ptr(), jv.data_ptr(), stream=stream())
        s = hv + jt
        torch.cuda.synchronize()
        return s.cpu().numpy(), jv.cpu().numpy()


# ---- 1. device == emulation, bit for bit ---------------------------------------------------------------------------------------------------
EMU_CASES = [("periodic", 2, False), ("periodic", 2, True), ("periodic", 3, False), ("periodic", 3, True), ("periodic", 4, False), ("periodic", 4, True),
             ("single", 3, False), ("cost_ends", 3, False), ("stairs", 3, False)]


@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("name,horizon,vary_first", EMU_CASES)
def test_device_equals_the_emulation_bitwise(model, name, horizon, vary_first, lifted):
    from kkt_emu_lib import KktEmu
    pr = Problem(model, name, horizon, batch=3, lifted=lifted, vary_first=vary_first, seed=horizon)
    emu = KktEmu(pr.st, model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
    assert (emu.n, emu.m, emu.nnz, emu.nnz_h) == (pr.eng.n, pr.eng.m, pr.eng.nnz, pr.eng.hess_nnz())
    hh, jh = pr.hess.cpu().numpy(), pr.jac.cpu().numpy()
    for dx, dc in ((True, True), (True, False), (False, False)):
        top, bottom = pr.kkt(dx=dx, dc=dc)
        for b in range(pr.B):
            et, eb, _, _ = emu.kkt_times(hh[b], jh[b], pr.v[b], pr.w[b], dx=pr.dx[b] if dx else None, dc=pr.dc[b] if dc else None)
            assert np.array_equal(bits(top[b]), bits(et)), ("top", dx, dc, b, np.flatnonzero(bits(top[b]) != bits(et))[:6])
            assert np.array_equal(bits(bottom[b]), bits(eb)), ("bottom", dx, dc, b, np.flatnonzero(bits(bottom[b]) != bits(eb))[:6])


# ---- 2. device == the three launches it replaces ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("name,horizon", [("periodic", 2), ("periodic", 3), ("cost_ends", 2), ("single", 3), ("stairs", 3)])
def test_device_equals_the_three_launches_bitwise(model, name, horizon, lifted):
    pr = Problem(model, name, horizon, batch=2, lifted=lifted, vary_first=True, seed=10 + horizon)
    s, jv = pr.three_launches()
    top, bottom = pr.kkt()
    assert np.array_equal(bits(top), bits(s)), np.argwhere(bits(top) != bits(s))[:6]
    assert np.array_equal(bits(bottom), bits(jv)), np.argwhere(bits(bottom) != bits(jv))[:6]
    top, bottom = pr.kkt(dx=True, dc=True)
    for b in range(pr.B):
        assert np.array_equal(bits(top[b]), bits(kkt_check.exact_fma(pr.dx[b], pr.v[b], s[b]))), ("top", b)
        assert np.array_equal(bits(bottom[b]), bits(kkt_check.exact_fma(-pr.dc[b], pr.w[b], jv[b]))), ("bottom", b)


# ---- 3. against the oracle -------------------------------------------------------------------------------------------------------------------
def against_oracle(model, name, horizon, lifted):
    from oracle_lib import Oracle
    smooth = name in SMOOTH
    tol = TOL_SMOOTH if smooth else TOL_PLANAR
    pr = Problem(model, name, horizon, batch=2, lifted=lifted, seed=20 + horizon)
    eng = pr.eng
    n, m = eng.n, eng.m
    top, bottom = pr.kkt(dx=True, dc=True)
    orc = Oracle(pr.st, model)
    iro, jco = orc.sparsity()
    ir, jc = eng.sparsity()
    hr, hc = eng.hess_sparsity()
    kept = eng.lift_map(with_bounds=False)[0]
    sel, mf = kept >= 0, kept.size
    k_h, k_c, k_r = hvp_check.touch_counts(hr, hc, n), lgrad_check.column_counts(jc, n), np.bincount(iro, minlength=mf)
    for b in range(pr.B):
        what = "%s N=%d lifted=%s b=%d" % (name, horizon, lifted, b)
        _, _, _, jaco = orc.eval(pr.x[b], pr.p[b])
        jaco = np.asarray(jaco)
        hro, hco, hvo = orc.hess(pr.x[b], pr.p[b], float(pr.sigma[b]), lgrad_check.full_multipliers(pr.lam[b], kept))
        w_full = lgrad_check.full_multipliers(pr.w[b], kept)
        ref_h, bound_h = hvp_check.oracle_bound(hro, hco, hvo, hr, hc, pr.v[b], k_h, smooth)
        ref_t, bound_t = lgrad_check.oracle_bound(np.zeros(n), iro, jco, jaco, 0.0, w_full, k_c, tol)
        dv = pr.dx[b] * pr.v[b]
        lgrad_check.check(top[b], ref_h + ref_t + dv, bound_h + bound_t + 2.0 ** -52 * np.abs(dv), what + ": top against the oracle")
        ref_j = row_times(iro, jco, jaco, pr.v[b], mf)
        bound_j = tol * row_times(iro, jco, jaco, pr.v[b], mf, floor=True) + 2.0 * gamma(k_r + 1) * row_times(iro, jco, jaco, pr.v[b], mf, absolute=True)
        dw = pr.dc[b] * pr.w[b]
        lgrad_check.check(bottom[b][kept[sel]], ref_j[sel] - dw[kept[sel]], bound_j[sel] + 2.0 ** -52 * np.abs(dw[kept[sel]]), what + ": bottom against the oracle")


@pytest.mark.parametrize("lifted", [False, True])
@pytest.mark.parametrize("horizon", [2, 3])
@pytest.mark.parametrize("planner", list(PLANNERS))
def test_matches_oracle_on_the_planners(model, planner, horizon, lifted):
    against_oracle(model, planner, horizon, lifted)


@pytest.mark.parametrize("lifted", [False, True])
def test_matches_oracle_on_the_ramp(model, lifted):
    against_oracle(model, "ramp", 3, lifted)


# ---- 4. destinations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,horizon", [("periodic", 3), ("cost_ends", 2), ("stairs", 4)])
def test_guard_words_and_omitted_diagonals(model, name, horizon):
    import torch
    pr = Problem(model, name, horizon, batch=3, seed=30 + horizon)
    eng, B, G = pr.eng, pr.B, 256
    s, jv = pr.three_launches()

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
    for dx, dc in ((0, 0), (pr.dxd.data_ptr(), pr.dcd.data_ptr())):
        top, bottom = guarded(B * eng.n), guarded(B * eng.m)
        eng.kkt_times_device(pr.hess.data_ptr(), pr.jac.data_ptr(), pr.vd.data_ptr(), pr.wd.data_ptr(), top.data_ptr() + 8 * G, bottom.data_ptr() + 8 * G,
                             dx_ptr=dx, dc_ptr=dc, stream=stream())
        torch.cuda.synchronize()
        t, bt = body(top, B * eng.n).reshape(B, eng.n), body(bottom, B * eng.m).reshape(B, eng.m)
        if not dx:   # the diagonals omitted: the bits of the three launches
            assert np.array_equal(bits(t), bits(s)) and np.array_equal(bits(bt), bits(jv))
        else:
            assert not np.array_equal(bits(t), bits(s)) and not np.array_equal(bits(bt), bits(jv))


# ---- 5. batch positions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,horizon", [("periodic", 4), ("cost_ends", 3)])
def test_batch_positions_give_the_same_bits(model, name, horizon):
    pr = Problem(model, name, horizon, batch=3, seed=40, same=True)
    hh, jh = pr.hess.cpu().numpy(), pr.jac.cpu().numpy()
    assert np.array_equal(bits(hh[0]), bits(hh[1])) and np.array_equal(bits(jh[0]), bits(jh[2]))
    top, bottom = pr.kkt(dx=True, dc=True)
    for b in (1, 2):
        assert np.array_equal(bits(top[b]), bits(top[0])) and np.array_equal(bits(bottom[b]), bits(bottom[0]))


# ---- 6. error codes ----------------------------------------------------------------------------------------------------------------------------
def test_error_codes(model):
    import torch
    from hippopt_amd.hipnlp import HipNlp, HipNlpError
    st = periodic_step_settings(6, model)
    x, p = make_workload(st, model, batch=1, seed=8600)
    plain = HipNlp(st, model)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    hess, jac, v, w = z(1, plain.hess_nnz()), z(1, plain.nnz), z(1, plain.n), z(1, plain.m)
    top, bottom = nans(1, plain.n), nans(1, plain.m)
    P = lambda t: t.data_ptr()  # noqa: E731
    args = [P(hess), P(jac), P(v), P(w), P(top), P(bottom)]
    for missing in range(6):
        a = list(args)
        a[missing] = 0
        with pytest.raises(HipNlpError) as e:
            plain.kkt_times_device(*a)
        assert e.value.code == -1                   # HIPNLP_E_INVALID
    front = HipNlp(st, model, devices=[0, 0])       # a two-shard front of device 0
    front.set_params(p)
    shard = HipNlp(st, model, knot_begin=0, knot_end=3)
    shard.set_params(p)
    for eng, word in ((front, "multi-device"), (shard, "shard")):
        with pytest.raises(HipNlpError) as e:
            eng.kkt_times_device(*args)
        assert e.value.code == -6 and word in str(e.value) and "hipnlp_kkt_times_device" in str(e.value)
    torch.cuda.synchronize()
    assert bool(torch.isnan(top).all()) and bool(torch.isnan(bottom).all())   # nothing was launched
    plain.kkt_times_device(*args)                   # (needs no parameters; zeros in, zeros out)
    torch.cuda.synchronize()
    assert not bool(top.any()) and not bool(bottom.any())


# ---- 7. torch ------------------------------------------------------------------------------------------------------------------------------------
def test_torch_kkt_values(model):
    import torch
    from hippopt_amd.autograd import KKTValues, KinodynamicNLP
    st = PLANNERS["cost_ends"](3, model)
    B = 2
    x, p = make_workload(st, model, batch=B, seed=8700)
    rng = np.random.RandomState(5)
    eq = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))  # noqa: E731
    for lifted in (False, True):
        nlp = KinodynamicNLP(st, model, batch=B, detect_simple_bounds=lifted)
        nlp.set_params(p)
        xd, lam = dev(x), dev(rng.standard_normal((B, nlp.m)))
        v, w = dev(rng.standard_normal((B, nlp.n))), dev(rng.standard_normal((B, nlp.m)))
        dx, dc = dev(rng.uniform(0.1, 3.0, (B, nlp.n))), dev(rng.uniform(0.1, 3.0, (B, nlp.m)))
        K = nlp.kkt(xd, 0.7, lam, dx, dc)
        assert K.hess.shape == (B, nlp.engine.hess_nnz()) and K.jac.shape == (B, nlp.engine.nnz) and K.dx is dx and K.dc is dc
        assert eq(K.hess, nlp.hessian(xd, 0.7, lam).values) and eq(K.jac, nlp.jacobian(xd).values)
        top, bottom = K.matvec(v, w)
        rt, rb = nans(B, nlp.n), nans(B, nlp.m)
        nlp.engine.kkt_times_device(K.hess.data_ptr(), K.jac.data_ptr(), v.data_ptr(), w.data_ptr(), rt.data_ptr(), rb.data_ptr(), dx_ptr=dx.data_ptr(), dc_ptr=dc.data_ptr(),
                                    stream=stream())
        torch.cuda.synchronize()
        assert eq(top, rt) and eq(bottom, rb)
        K0 = K.with_diagonals(None, None)
        assert K0.hess.data_ptr() == K.hess.data_ptr() and K0.jac.data_ptr() == K.jac.data_ptr() and K0.dx is None and K0.dc is None
        t0, b0 = K0.matvec(v, w)
        H, J = nlp.hessian(xd, 0.7, lam), nlp.jacobian(xd)
        K1 = KKTValues(nlp, H, J, dx=dx)           # from objects the caller already holds
        assert K1.hess.data_ptr() == H.values.data_ptr() and K1.jac.data_ptr() == J.values.data_ptr()
        t1, b1 = K1.matvec(v, w)
        assert eq(t1, top) and eq(b1, J.matvec(v)) and eq(b0, b1)
        assert not top.requires_grad
    # on a stream of the caller's: the same bits, ordered on that stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Ks = nlp.kkt(dev(x), 0.7, lam, dx, dc)
        ts, bs = Ks.matvec(v, w)
        same = eq(ts, top) and eq(bs, bottom)
    side.synchronize()
    assert same


def test_torch_binding_refuses_wrong_tensors(model):
    import torch
    from hippopt_amd.autograd import KKTValues, KinodynamicNLP
    st = periodic_step_settings(3, model)
    B = 2
    x, p = make_workload(st, model, batch=B, seed=8800)
    nlp = KinodynamicNLP(st, model, batch=B)
    nlp.set_params(p)
    good = torch.tensor(x, device="cuda")
    lam = torch.zeros((B, nlp.m), dtype=torch.float64, device="cuda")
    K = nlp.kkt(good, 1.0, lam)
    wide_n, wide_m = torch.zeros((B, 2 * nlp.n), dtype=torch.float64, device="cuda"), torch.zeros((B, 2 * nlp.m), dtype=torch.float64, device="cuda")
    bad_n = [(TypeError, good.float()), (ValueError, good.cpu()), (ValueError, good[:1]), (ValueError, wide_n[:, ::2])]
    bad_m = [(TypeError, lam.float()), (ValueError, lam.cpu()), (ValueError, lam[:1]), (ValueError, lam[:, :-1]), (ValueError, wide_m[:, ::2])]
    for exc, t in bad_n:
        for call in (lambda: K.matvec(t, lam), lambda: K.with_diagonals(t, None), lambda: nlp.kkt(t, 1.0, lam), lambda: nlp.kkt(good, 1.0, lam, dx=t)):
            with pytest.raises(exc):
                call()
    for exc, t in bad_m:
        for call in (lambda: K.matvec(good, t), lambda: K.with_diagonals(None, t), lambda: nlp.kkt(good, 1.0, t), lambda: nlp.kkt(good, 1.0, lam, dc=t)):
            with pytest.raises(exc):
                call()
    for exc, t in ((TypeError, K.hess.float()), (ValueError, K.hess[:, :-1])):
        with pytest.raises(exc):
            KKTValues(nlp, t, K.jac)
    for exc, t in ((TypeError, K.jac.float()), (ValueError, K.jac[:, :-1])):
        with pytest.raises(exc):
            KKTValues(nlp, K.hess, t)
