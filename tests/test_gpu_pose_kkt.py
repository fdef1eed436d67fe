"""GPU: the KKT chain of the pose finder from stored value runs, one launch each (hipnlp_pose_kkt_times_device,
hipnlp_pose_kkt_diag_precond_device, hipnlp_pose_kkt_minres_device; the kernels hipnlp_pose_saddle_*_kernel of hipnlp_pose.hip) and
hippopt_amd.autograd.PoseNLP.kkt built on them.  Every output equals the CPU emulation of the kernels (tests/pose_kkt_emu) BIT FOR BIT, for
all six settings variants, on the synthetic inputs of pose_kkt_check.inputs and on the handle's own real value runs; what the numbers are
worth is checked on the emulation (test_pose_kkt_hostemu.py).  Batch 3; every destination is NaN-filled between guard words."""
import numpy as np
import pytest

import pose_kkt_check as pkc
import pose_products_check as ppc
from test_pose_body_hostemu import VARIANTS, variants

pytestmark = pytest.mark.gpu
B = 3
GUARD = 64
_CASE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev(a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """a destination of `shape` between two runs of guard words; float64 starts as NaN, int32 as -99"""

    def __init__(self, shape, integer=False):
        import torch
        n = int(np.prod(shape))
        self.mark = 1234 if integer else 1234.5
        self.buf = torch.full((n + 2 * GUARD,), -99 if integer else float("nan"), dtype=torch.int32 if integer else torch.float64, device="cuda")
        self.buf[:GUARD] = self.mark
        self.buf[GUARD + n:] = self.mark
        self.body = self.buf[GUARD:GUARD + n].view(*shape)
        torch.cuda.synchronize()          # (the fills run on torch's stream, the raw calls on the handle's own)

    def ptr(self):
        return self.body.data_ptr()

    def get(self):
        """the body as a numpy array; asserts that the guard words are what they were"""
        h = self.buf.cpu().numpy()
        assert np.all(h[:GUARD] == self.mark) and np.all(h[-GUARD:] == self.mark), "guard words overwritten"
        return self.body.cpu().numpy().copy()


class Case:
    """one handle of a variant (batch 3), its emulation, and its two batches of systems: `syn` (pose 0: synthetic 0.05, pose 1: synthetic
    0.02, pose 2: pose 0 rescaled to cond about 1e12) and `real` (the handle's own value runs at the three poses of the workload)"""

    def __init__(self, model, name):
        import torch
        from hippopt_amd.hipnlp import HipPose
        from pose_kkt_emu_lib import PoseKktEmu
        st = variants(model)[name]
        self.eng, self.emu = HipPose(st, model, batch=B), PoseKktEmu(st, model)
        e = self.emu
        ir, jc, hr, hc = e.sparsity()
        self.pat = (hr, hc, ir, jc)
        self.x, p = ppc.workload(name, st, model, pkc.WORKLOAD_SEED)
        self.eng.set_params(p)
        self.lam, self.sigma, _ = ppc.factors(e.m, e.n, pkc.FACTOR_SEED)
        syn, real = pkc.inputs(e.n, e.m, e.nnz, e.hnnz)
        keys = ("hess", "jac", "dx", "dc", "bt", "bb")
        self.syn = {k: np.stack([syn[0][k], syn[1][k], pkc.rescaled(syn[0], self.pat)[k]]) for k in keys}
        self.syn["mt"], self.syn["mb"] = (np.stack([syn[0][k], syn[1][k], syn[0][k]]) for k in ("mt", "mb"))
        jac, hess = Guarded((B, e.nnz)), Guarded((B, e.hnnz))
        xd, sd, ld = dev(self.x), dev(self.sigma), dev(self.lam)
        self.eng.eval_device(xd.data_ptr(), 0, 0, 0, jac.ptr(), stream=_stream())
        self.eng.eval_hess_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), hess.ptr(), stream=_stream())
        torch.cuda.synchronize()
        self.real = {k: np.stack([real[b][k] for b in range(B)]) for k in ("dx", "dc", "bt", "bb")}
        self.real.update(jac=jac.get(), hess=hess.get(), mt=self.syn["mt"], mb=self.syn["mb"])
        assert np.all(np.isfinite(self.real["jac"])) and np.all(np.isfinite(self.real["hess"]))

    # ---- the device calls on numpy batches: every destination guarded -----------------------------------------------------------------
    def times(self, d, v, w, dx, dc):
        import torch
        top, bottom = Guarded((B, self.emu.n)), Guarded((B, self.emu.m))
        t = [dev(a) for a in (d["hess"], d["jac"], v, w, dx, dc)]
        self.eng.kkt_times_device(ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), top.ptr(), bottom.ptr(), dx_ptr=ptr(t[4]), dc_ptr=ptr(t[5]), stream=_stream())
        torch.cuda.synchronize()
        return top.get(), bottom.get()

    def diag(self, d, dx, dc, floor=1e-10):
        import torch
        top, bottom = Guarded((B, self.emu.n)), Guarded((B, self.emu.m))
        t = [dev(a) for a in (d["hess"], d["jac"], dx, dc)]
        self.eng.kkt_diag_precond_device(ptr(t[0]), ptr(t[1]), top.ptr(), bottom.ptr(), dx_ptr=ptr(t[2]), dc_ptr=ptr(t[3]), floor=floor, stream=_stream())
        torch.cuda.synchronize()
        return top.get(), bottom.get()

    def solve(self, d, bt, bb, dx, dc, minv, maxiter, floor=1e-10, rtol=1e-8):
        """(top, bottom, iterations, residual, status)"""
        import torch
        out = [Guarded((B, self.emu.n)), Guarded((B, self.emu.m)), Guarded((B,), integer=True), Guarded((B,)), Guarded((B,), integer=True)]
        build = isinstance(minv, str)
        mt, mb = (None, None) if (minv is None or build) else minv
        t = [dev(a) for a in (d["hess"], d["jac"], bt, bb, dx, dc, mt, mb)]
        self.eng.kkt_minres_device(ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), out[0].ptr(), out[1].ptr(), out[2].ptr(), out[3].ptr(), out[4].ptr(), dx_ptr=ptr(t[4]),
                                   dc_ptr=ptr(t[5]), minv_top_ptr=ptr(t[6]), minv_bottom_ptr=ptr(t[7]), build_diagonal=build, floor=floor, rtol=rtol, max_iterations=maxiter,
                                   stream=_stream())
        torch.cuda.synchronize()
        return tuple(o.get() for o in out)

    def emu_solve(self, d, b, bt, bb, dx, dc, minv, maxiter, floor=1e-10, rtol=1e-8):
        pick = lambda a: None if a is None else a[b]  # noqa: E731
        mv = minv if (minv is None or isinstance(minv, str)) else (minv[0][b], minv[1][b])
        return self.emu.solve(d["hess"][b], d["jac"][b], bt[b], bb[b], pick(dx), pick(dc), minv=mv, floor=floor, rtol=rtol, maxiter=maxiter)


def case_of(model, name):
    if name not in _CASE:
        _CASE[name] = Case(model, name)
    return _CASE[name]


def same_solution(got, b, sol):
    return (np.array_equal(bits(got[0][b]), bits(sol.top)) and np.array_equal(bits(got[1][b]), bits(sol.bottom)) and int(got[2][b]) == sol.iterations
            and bits([got[3][b]])[0] == bits([sol.residual])[0] and int(got[4][b]) == sol.status)


# ---- 1. the operator and the diagonal against the emulation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("diagonals", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("name", VARIANTS)
def test_operator_equals_the_emulation(model, name, diagonals):
    c = case_of(model, name)
    rng = np.random.RandomState(77)
    for what, d in (("synthetic", c.syn), ("real", c.real)):
        v, w = rng.standard_normal((B, c.emu.n)), rng.standard_normal((B, c.emu.m))
        dx, dc = (d["dx"] if diagonals[0] else None), (d["dc"] if diagonals[1] else None)
        top, bottom = c.times(d, v, w, dx, dc)
        for b in range(B):
            ref = c.emu.times(d["hess"][b], d["jac"][b], v[b], w[b], None if dx is None else dx[b], None if dc is None else dc[b])
            assert np.array_equal(bits(top[b]), bits(ref.top)) and np.array_equal(bits(bottom[b]), bits(ref.bottom)), (what, b)


@pytest.mark.parametrize("diagonals", [(True, True), (False, False)])
@pytest.mark.parametrize("name", VARIANTS)
def test_diagonal_equals_the_emulation(model, name, diagonals):
    c = case_of(model, name)
    for what, d, floor in (("synthetic", c.syn, 1e-300), ("real", c.real, 1e-10)):
        dx, dc = (d["dx"] if diagonals[0] else None), (d["dc"] if diagonals[1] else None)
        top, bottom = c.diag(d, dx, dc, floor)
        for b in range(B):
            ref = c.emu.diagonal_preconditioner(d["hess"][b], d["jac"][b], None if dx is None else dx[b], None if dc is None else dc[b], floor)
            assert np.array_equal(bits(top[b]), bits(ref.top)) and np.array_equal(bits(bottom[b]), bits(ref.bottom)), (what, b)


# ---- 2. the solve against the emulation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minv", ["identity", "given", "diagonal"])
@pytest.mark.parametrize("name", VARIANTS)
def test_solve_equals_the_emulation(model, name, minv):
    """all five outputs, whatever the status: on the synthetic batch pose 2 (cond 1e12) ends at the limit without the built diagonal;
    on the real batch the identity and the random diagonal end at the limit, the built diagonal converges"""
    c = case_of(model, name)
    for what, d, maxiter, floor in (("synthetic", c.syn, 100, 1e-300), ("real", c.real, 400 if minv == "diagonal" else 120, 1e-10)):
        mv = None if minv == "identity" else ((d["mt"], d["mb"]) if minv == "given" else "diagonal")
        got = c.solve(d, d["bt"], d["bb"], d["dx"], d["dc"], mv, maxiter, floor)
        print("%s %s minv=%s: iterations %s status %s residual %s" % (name, what, minv, got[2], got[4], got[3]))
        for b in range(B):
            assert same_solution(got, b, c.emu_solve(d, b, d["bt"], d["bb"], d["dx"], d["dc"], mv, maxiter, floor)), (what, b)
        if minv == "diagonal":
            assert np.all(got[4] == 0), (what, got[4])                   # (the emulation's own test: all converge)


@pytest.mark.parametrize("name", ["default", "hands_steps"])
def test_omitted_diagonals_and_build_diagonal_is_the_preconditioner_call(model, name):
    c = case_of(model, name)
    d = c.real
    for dx, dc in ((None, d["dc"]), (d["dx"], None), (None, None)):
        got = c.solve(d, d["bt"], d["bb"], dx, dc, "diagonal", 40, 1e-9)
        for b in range(B):
            assert same_solution(got, b, c.emu_solve(d, b, d["bt"], d["bb"], dx, dc, "diagonal", 40, 1e-9)), b
        two = c.solve(d, d["bt"], d["bb"], dx, dc, c.diag(d, dx, dc, 1e-9), 40)
        for a, t in zip(got, two):
            assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(t) if t.dtype == np.float64 else t)


# ---- 3. against the fused products of the same handle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_operator_against_the_fused_products(model, name):
    """w = 0 and no dx: top is H v of hipnlp_pose_eval_hess_vec_device at the same (x, sigma, lam, v) — the same touches in the same order
    plus a column sum of zeros; no dc: bottom is J v of hipnlp_pose_eval_jac_vec_device bit for bit"""
    import torch
    c = case_of(model, name)
    v = np.random.RandomState(78).standard_normal((B, c.emu.n))
    top, bottom = c.times(c.real, v, np.zeros((B, c.emu.m)), None, None)
    hv, jv = Guarded((B, c.emu.n)), Guarded((B, c.emu.m))
    xd, sd, ld, vd = dev(c.x), dev(c.sigma), dev(c.lam), dev(v)
    c.eng.eval_hess_vec_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), vd.data_ptr(), hv.ptr(), stream=_stream())
    c.eng.eval_jac_vec_device(xd.data_ptr(), vd.data_ptr(), 0, jv.ptr(), stream=_stream())
    torch.cuda.synchronize()
    assert np.array_equal(top, hv.get())
    assert np.array_equal(bits(bottom), bits(jv.get()))


# ---- 4. batch positions, independence of the poses of a batch -------------------------------------------------------------------------------------
def test_the_same_pose_at_every_batch_position_gives_the_same_bits(model):
    c = case_of(model, "steps")
    rng = np.random.RandomState(79)
    d = {k: np.stack([a[0]] * B) for k, a in c.real.items()}
    v, w = np.stack([rng.standard_normal(c.emu.n)] * B), np.stack([rng.standard_normal(c.emu.m)] * B)
    outs = c.times(d, v, w, d["dx"], d["dc"]) + c.diag(d, d["dx"], d["dc"]) + c.solve(d, d["bt"], d["bb"], d["dx"], d["dc"], "diagonal", 400)
    for a in outs:
        assert np.all(np.isfinite(a))
        for b in range(1, B):
            assert np.array_equal(bits(a[b]) if a.dtype == np.float64 else a[b], bits(a[0]) if a.dtype == np.float64 else a[0])


def test_a_zero_right_hand_side_and_a_pose_at_the_limit_leave_the_others_alone(model):
    c = case_of(model, "hands")
    d = c.syn
    bt, bb = d["bt"].copy(), d["bb"].copy()
    bt[1], bb[1] = 0.0, 0.0
    plain = c.solve(d, d["bt"], d["bb"], d["dx"], d["dc"], None, 60)
    got = c.solve(d, bt, bb, d["dx"], d["dc"], None, 60)
    print("iterations %s status %s residual %s" % (got[2], got[4], got[3]))
    assert (int(got[2][1]), int(got[4][1]), float(got[3][1])) == (0, 0, 0.0) and not got[0][1].any() and not got[1][1].any()      # b = 0
    assert (int(got[2][2]), int(got[4][2])) == (60, 1)                                                                             # cond 1e12, identity
    assert int(got[4][0]) == 0 and 0 < int(got[2][0]) < 60
    for b in (0, 2):
        for a, t in zip(got, plain):
            assert np.array_equal(bits(a[b]) if a.dtype == np.float64 else a[b], bits(t[b]) if t.dtype == np.float64 else t[b])
    for b in range(B):
        assert same_solution(got, b, c.emu_solve(d, b, bt, bb, d["dx"], d["dc"], None, 60))


def test_solves_on_two_streams_are_independent(model):
    """no workspace: two solves of one handle in flight on two streams give the bits each gives alone"""
    import torch
    c = case_of(model, "constrained")
    d = c.real
    alone = [c.solve(d, bt, d["bb"], d["dx"], d["dc"], "diagonal", 400) for bt in (d["bt"], -2.0 * d["bt"])]
    t = {k: dev(d[k]) for k in ("hess", "jac", "bb", "dx", "dc")}
    rhs = [dev(d["bt"]), dev(-2.0 * d["bt"])]
    outs = [[Guarded((B, c.emu.n)), Guarded((B, c.emu.m)), Guarded((B,), integer=True), Guarded((B,)), Guarded((B,), integer=True)] for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for s, bt, o in zip(streams, rhs, outs):
        c.eng.kkt_minres_device(ptr(t["hess"]), ptr(t["jac"]), ptr(bt), ptr(t["bb"]), o[0].ptr(), o[1].ptr(), o[2].ptr(), o[3].ptr(), o[4].ptr(), dx_ptr=ptr(t["dx"]),
                                dc_ptr=ptr(t["dc"]), build_diagonal=True, max_iterations=400, stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o, ref in zip(outs, alone):
        for a, r in zip((q.get() for q in o), ref):
            assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(r) if r.dtype == np.float64 else r)
    assert not np.array_equal(alone[0][0], alone[1][0])


def test_invalid_arguments_on_a_live_handle(model):
    """HIPNLP_E_INVALID before anything is launched: null required pointers, a floor that is not a finite number > 0, rtol < 0,
    max_iterations outside 0 .. 4096, one of minv_top / minv_bottom alone or either with build_diagonal; the destinations stay NaN"""
    import torch
    from hippopt_amd import _abi
    from hippopt_amd.hipnlp import HipNlpError
    c = case_of(model, "default")
    d = c.syn
    t = {k: dev(d[k]) for k in ("hess", "jac", "bt", "bb", "dx", "dc", "mt", "mb")}
    out = [Guarded((B, c.emu.n)), Guarded((B, c.emu.m)), Guarded((B,), integer=True), Guarded((B,)), Guarded((B,), integer=True)]
    good = [ptr(t["hess"]), ptr(t["jac"]), ptr(t["bt"]), ptr(t["bb"])] + [o.ptr() for o in out]

    def refused(call):
        with pytest.raises(HipNlpError) as err:
            call()
        assert err.value.code == _abi.E_INVALID, err.value

    for i in range(9):                                                                                   # every required pointer of the solve
        refused(lambda: c.eng.kkt_minres_device(*(good[:i] + [0] + good[i + 1:]), stream=_stream()))
    for kw in (dict(max_iterations=4097), dict(max_iterations=-1), dict(rtol=-1e-8), dict(rtol=float("nan")), dict(floor=0.0), dict(floor=float("inf")), dict(floor=float("nan")),
               dict(minv_top_ptr=ptr(t["mt"])), dict(minv_bottom_ptr=ptr(t["mb"])), dict(minv_top_ptr=ptr(t["mt"]), minv_bottom_ptr=ptr(t["mb"]), build_diagonal=True)):
        refused(lambda: c.eng.kkt_minres_device(*good, stream=_stream(), **kw))
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: c.eng.kkt_diag_precond_device(good[0], good[1], out[0].ptr(), out[1].ptr(), floor=floor, stream=_stream()))
    refused(lambda: c.eng.kkt_diag_precond_device(good[0], good[1], 0, out[1].ptr(), stream=_stream()))
    refused(lambda: c.eng.kkt_times_device(good[0], good[1], good[2], 0, out[0].ptr(), out[1].ptr(), stream=_stream()))
    refused(lambda: c.eng.kkt_times_device(good[0], 0, good[2], good[3], out[0].ptr(), out[1].ptr(), stream=_stream()))
    torch.cuda.synchronize()
    assert np.all(np.isnan(out[0].get())) and np.all(np.isnan(out[1].get())) and np.all(np.isnan(out[3].get())) and np.all(out[2].get() == -99) and np.all(out[4].get() == -99)
    c.eng.kkt_minres_device(*good, max_iterations=4096, rtol=0.0, stream=_stream())                      # the limits themselves are valid
    torch.cuda.synchronize()
    assert np.all(out[4].get() >= 0)


# ---- 5. torch -------------------------------------------------------------------------------------------------------------------------------
def test_pose_nlp_kkt_equals_the_raw_calls_and_solves_the_system(model):
    import torch
    from hippopt_amd.autograd import KKTSolution, PoseKKTValues, PoseNLP
    name = "hands_steps"
    c = case_of(model, name)
    st = variants(model)[name]
    _, p = ppc.workload(name, st, model, pkc.WORKLOAD_SEED)
    nlp = PoseNLP(st, model, batch=B)
    nlp.set_params(p)
    d = c.real
    dx, dc, bt, bb = (dev(d[k]) for k in ("dx", "dc", "bt", "bb"))
    K = nlp.kkt(dev(c.x), dev(c.sigma), dev(c.lam), dx, dc)
    assert isinstance(K, PoseKKTValues)
    assert np.array_equal(bits(K.hess.cpu().numpy()), bits(d["hess"])) and np.array_equal(bits(K.jac.cpu().numpy()), bits(d["jac"]))
    z = K.solve(bt, bb, rtol=1e-8, maxiter=400, minv="diagonal")
    assert isinstance(z, KKTSolution)
    raw = c.solve(d, d["bt"], d["bb"], d["dx"], d["dc"], "diagonal", 400)
    for a, t in zip(z, raw):
        a = a.cpu().numpy()
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(t) if t.dtype == np.float64 else t)
    pair = K.diagonal_preconditioner()
    z2 = K.solve(bt, bb, minv=pair)
    assert torch.equal(z2.top, z.top) and torch.equal(z2.bottom, z.bottom) and torch.equal(z2.iterations, z.iterations)
    top, bottom = K.matvec(z.top, z.bottom)
    r = torch.cat([top - bt, bottom - bb], dim=1)
    mi = torch.cat(pair, dim=1)
    rel = (torch.sqrt((r * mi * r).sum(1)) / torch.sqrt((torch.cat([bt, bb], 1) ** 2 * mi).sum(1))).cpu().numpy()
    print("status %s iterations %s residual %s, sqrt(r . M^-1 r) / sqrt(b . M^-1 b) through matvec %s" % (z.status.cpu().numpy(), z.iterations.cpu().numpy(), z.residual.cpu().numpy(), rel))
    assert np.all(z.status.cpu().numpy() == 0) and np.all(z.residual.cpu().numpy() <= 1e-8)
    assert np.all(np.abs(rel - z.residual.cpu().numpy()) <= 1e-8)      # (the estimate against the true residual: the bound of tests/test_kkt_minres_hostemu.py)
    t0, b0 = K.with_diagonals(None, None).matvec(z.top, z.bottom)      # the same value runs without the diagonals: no evaluation launch
    assert not torch.equal(t0, top) and not torch.equal(b0, bottom)
