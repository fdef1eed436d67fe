"""GPU: the dense L D L^T of the pose finder's KKT matrix, one launch (hipnlp_pose_kkt_ldl_device, hipnlp_pose_kkt_ldl_solve_device; the
kernels hipnlp_pose_saddle_ldl_kernel and hipnlp_pose_saddle_ldl_solve_kernel of hipnlp_pose.hip) and hippopt_amd.autograd.PoseKKTValues.factor /
solve_direct built on them.  Solutions, factor, pivots, inertia, status, delta and tries equal the CPU emulation (tests/pose_ldl_emu, which
walks the elements in another order) BIT FOR BIT, for all six settings variants, on the synthetic batch (with the rescaled pose) and on
the handle's own real value runs, with and without dx / dc, for nrhs 0, 1 and 3, with the ladder's case, a singular pose and a NaN pose
between good ones; what the numbers are worth is checked on the emulation (test_pose_ldl_hostemu.py).  Batch 3; every destination is
NaN-filled between guard words."""
import numpy as np
import pytest

import pose_kkt_check as pkc
import pose_ldl_check as plc
import pose_products_check as ppc
from test_pose_body_hostemu import VARIANTS, variants

pytestmark = pytest.mark.gpu
B = 3
GUARD = 64
_CASE = {}
LADDER = dict(delta_init=plc.DELTA_INIT, kappa=plc.KAPPA, max_tries=16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev(a, integer=False):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.int32 if integer else torch.float64, device="cuda")


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
        from pose_ldl_emu_lib import PoseLdlEmu
        st = variants(model)[name]
        self.eng, self.emu = HipPose(st, model, batch=B), PoseLdlEmu(st, model)
        e = self.emu
        ir, jc, hr, hc = e.sparsity()
        self.pat = (hr, hc, ir, jc)
        self.x, p = ppc.workload(name, st, model, pkc.WORKLOAD_SEED)
        self.eng.set_params(p)
        self.lam, self.sigma, _ = ppc.factors(e.m, e.n, pkc.FACTOR_SEED)
        syn, real = pkc.inputs(e.n, e.m, e.nnz, e.hnnz)
        keys = ("hess", "jac", "dx", "dc", "bt", "bb")
        self.syn = {k: np.stack([syn[0][k], syn[1][k], pkc.rescaled(syn[0], self.pat)[k]]) for k in keys}
        jac, hess = Guarded((B, e.nnz)), Guarded((B, e.hnnz))
        xd, sd, ld = dev(self.x), dev(self.sigma), dev(self.lam)
        self.eng.eval_device(xd.data_ptr(), 0, 0, 0, jac.ptr(), stream=_stream())
        self.eng.eval_hess_device(xd.data_ptr(), sd.data_ptr(), ld.data_ptr(), hess.ptr(), stream=_stream())
        torch.cuda.synchronize()
        self.real = {k: np.stack([real[b][k] for b in range(B)]) for k in ("dx", "dc", "bt", "bb")}
        self.real.update(jac=jac.get(), hess=hess.get())
        assert np.all(np.isfinite(self.real["jac"])) and np.all(np.isfinite(self.real["hess"]))
        assert self.eng.kkt_ldl_doubles() == e.doubles

    def rhs(self, d, nrhs):
        """(top [B, nrhs, 81], bottom [B, nrhs, m]): the system's own right-hand side first, then seeded ones"""
        if nrhs == 0:
            return None, None
        rng = np.random.RandomState(90 + nrhs)
        top = np.stack([d["bt"]] + [rng.standard_normal(d["bt"].shape) for _ in range(nrhs - 1)], 1)
        bottom = np.stack([d["bb"]] + [rng.standard_normal(d["bb"].shape) for _ in range(nrhs - 1)], 1)
        return top, bottom

    # ---- the device calls on numpy batches: every destination guarded -----------------------------------------------------------------
    def factor(self, d, dx, dc, top, bottom, store=True, **ladder):
        """dict top, bottom, inertia, status, delta, tries, factor, pivots (numpy; None where not asked for)"""
        import torch
        e = self.emu
        nrhs = 0 if top is None else top.shape[1]
        out = dict(inertia=Guarded((B, 3), integer=True), status=Guarded((B,), integer=True), delta=Guarded((B,)), tries=Guarded((B,), integer=True))
        if nrhs:
            out.update(top=Guarded((B, nrhs, e.n)), bottom=Guarded((B, nrhs, e.m)))
        if store:
            out.update(factor=Guarded((B, e.doubles)), pivots=Guarded((B, e.N), integer=True))
        t = [dev(a) for a in (d["hess"], d["jac"], dx, dc, top, bottom)]
        g = lambda k: out[k].ptr() if k in out else 0  # noqa: E731
        self.eng.kkt_ldl_device(ptr(t[0]), ptr(t[1]), g("inertia"), g("status"), dx_ptr=ptr(t[2]), dc_ptr=ptr(t[3]), nrhs=nrhs, rhs_top_ptr=ptr(t[4]), rhs_bottom_ptr=ptr(t[5]),
                                sol_top_ptr=g("top"), sol_bottom_ptr=g("bottom"), delta_ptr=g("delta"), tries_ptr=g("tries"), factor_ptr=g("factor"), pivots_ptr=g("pivots"),
                                stream=_stream(), **ladder)
        torch.cuda.synchronize()
        return {k: v.get() for k, v in out.items()}

    def solve(self, factor, pivots, top, bottom):
        import torch
        nrhs = top.shape[1]
        st, sb = Guarded((B, nrhs, self.emu.n)), Guarded((B, nrhs, self.emu.m))
        t = [dev(factor), dev(pivots, integer=True), dev(top), dev(bottom)]
        self.eng.kkt_ldl_solve_device(ptr(t[0]), ptr(t[1]), nrhs, ptr(t[2]), ptr(t[3]), st.ptr(), sb.ptr(), stream=_stream())
        torch.cuda.synchronize()
        return st.get(), sb.get()

    def emu_factor(self, d, b, dx, dc, top, bottom, **ladder):
        pick = lambda a: None if a is None else a[b]  # noqa: E731
        return self.emu.factor(d["hess"][b], d["jac"][b], pick(dx), pick(dc), pick(top), pick(bottom), **ladder)


def case_of(model, name):
    if name not in _CASE:
        _CASE[name] = Case(model, name)
    return _CASE[name]


def assert_same(got, b, ref, what):
    """every output of pose b against the emulation's Factored, bit for bit (a NaN is a NaN: status 1 and 2 give NaN solutions, and a
    NaN of the data may sit in the factor)"""
    assert (tuple(int(v) for v in got["inertia"][b]), int(got["status"][b]), int(got["tries"][b])) == (ref.inertia, ref.status, ref.tries), (what, b)
    assert bits([got["delta"][b]])[0] == bits([ref.delta])[0], (what, b)
    if "top" in got:
        if ref.status in (1, 2):
            assert np.all(np.isnan(got["top"][b])) and np.all(np.isnan(got["bottom"][b])) and np.all(np.isnan(ref.top)) and np.all(np.isnan(ref.bottom)), (what, b)
        else:
            assert np.array_equal(bits(got["top"][b]), bits(ref.top)) and np.array_equal(bits(got["bottom"][b]), bits(ref.bottom)), (what, b)
        assert np.all(ref.top_writes == 1) and np.all(ref.bottom_writes == 1)
    if "factor" in got:
        assert np.array_equal(got["pivots"][b], ref.pivots), (what, b)
        if ref.status == 2:
            assert np.array_equal(got["factor"][b], ref.factor, equal_nan=True), (what, b)
        else:
            assert np.array_equal(bits(got["factor"][b]), bits(ref.factor)), (what, b)


# ---- 1. everything against the emulation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diagonals", [(True, True), (False, True), (False, False)])
@pytest.mark.parametrize("name", VARIANTS)
def test_factor_inertia_and_solves_equal_the_emulation(model, name, diagonals):
    c = case_of(model, name)
    for what, d in (("synthetic", c.syn), ("real", c.real)):
        dx, dc = (d["dx"] if diagonals[0] else None), (d["dc"] if diagonals[1] else None)
        for nrhs in (0, 1, 3):
            top, bottom = c.rhs(d, nrhs)
            got = c.factor(d, dx, dc, top, bottom, store=nrhs != 1)
            print("%s %s diagonals %s nrhs %d: status %s inertia %s" % (name, what, diagonals, nrhs, got["status"], got["inertia"].tolist()))
            for b in range(B):
                assert_same(got, b, c.emu_factor(d, b, dx, dc, top, bottom), (what, nrhs))
    if diagonals == (True, True):
        assert np.all(got["status"] == 0)


# ---- 2. the ladder, a singular pose and a NaN pose between two good ones ---------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_ladder_singular_and_nan_poses_between_good_ones(model, name):
    c = case_of(model, name)
    e = c.emu
    good = c.syn
    one = lambda k: {q: a[k] for q, a in good.items()}  # noqa: E731
    top, bottom = c.rhs(good, 1)
    plain = c.factor(good, good["dx"], good["dc"], top, bottom, **LADDER)
    assert np.all(plain["status"] == 0) and np.all(plain["tries"] == 0) and np.all(plain["delta"] == 0.0)
    nodc = c.factor(good, good["dx"], None, top, bottom)
    for label, middle, dc, ladder, base in (("ladder", plc.indefinite(one(0)), good["dc"], LADDER, plain), ("nan", plc.with_nan(one(1)), good["dc"], LADDER, plain),
                                            ("singular", plc.singular(one(1)), None, {}, nodc)):
        d = {k: a.copy() for k, a in good.items()}
        for k in ("hess", "jac", "dx"):
            d[k][1] = middle[k]
        got = c.factor(d, d["dx"], dc, top, bottom, **ladder)
        print("%s %s: status %s tries %s delta %s inertia %s" % (name, label, got["status"], got["tries"], got["delta"], got["inertia"].tolist()))
        for b in range(B):
            assert_same(got, b, c.emu_factor(d, b, d["dx"], dc, top, bottom, **ladder), label)
        for b in (0, 2):                                                        # the neighbours: the bits of the batch without the odd pose
            for k in got:
                assert np.array_equal(got[k][b], base[k][b], equal_nan=True) and (got[k].dtype != np.float64 or np.array_equal(bits(got[k][b]), bits(base[k][b]))), (label, k, b)
        if label == "ladder":
            walk = plc.numpy_ladder(e, c.pat, plc.indefinite(one(0)))
            assert walk is not None and walk[0] >= 1
            assert (int(got["status"][1]), int(got["tries"][1]), float(got["delta"][1])) == (0, walk[0], walk[1]) and tuple(got["inertia"][1]) == (e.n, e.m, 0)
            short = c.factor(d, d["dx"], dc, top, bottom, delta_init=plc.DELTA_INIT, kappa=plc.KAPPA, max_tries=walk[0] - 1)
            assert short["status"].tolist() == [0, 3, 0] and int(short["tries"][1]) == walk[0] - 1
            assert_same(short, 1, c.emu_factor(d, 1, d["dx"], dc, top, bottom, delta_init=plc.DELTA_INIT, kappa=plc.KAPPA, max_tries=walk[0] - 1), "short ladder")
            once = c.factor(d, d["dx"], dc, top, bottom)
            assert int(once["status"][1]) == 0 and tuple(once["inertia"][1]) != (e.n, e.m, 0)
        elif label == "nan":
            assert got["status"].tolist() == [0, 2, 0] and np.all(np.isnan(got["top"][1])) and np.all(np.isnan(got["bottom"][1]))
        else:
            assert int(got["status"][1]) == 1 and int(got["inertia"][1][2]) >= 1 and np.all(np.isnan(got["top"][1]))


# ---- 3. the stored factor ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_a_solve_from_the_stored_factor_equals_the_fused_solve(model, name):
    c = case_of(model, name)
    for what, d in (("synthetic", c.syn), ("real", c.real)):
        for nrhs in (1, 3):
            top, bottom = c.rhs(d, nrhs)
            fused = c.factor(d, d["dx"], d["dc"], top, bottom)
            st, sb = c.solve(fused["factor"], fused["pivots"], top, bottom)
            assert np.array_equal(bits(st), bits(fused["top"])) and np.array_equal(bits(sb), bits(fused["bottom"])), (what, nrhs)
            for b in range(B):
                et, eb = c.emu.solve(fused["factor"][b], fused["pivots"][b], top[b], bottom[b])
                assert np.array_equal(bits(st[b]), bits(et)) and np.array_equal(bits(sb[b]), bits(eb)), (what, nrhs, b)


def test_the_same_pose_at_every_batch_position_gives_the_same_bits(model):
    c = case_of(model, "steps")
    d = {k: np.stack([a[0]] * B) for k, a in c.real.items()}
    top, bottom = (np.stack([a[0]] * B) for a in c.rhs(d, 3))
    got = c.factor(d, d["dx"], d["dc"], top, bottom)
    for k, a in got.items():
        assert np.all(np.isfinite(a)), k
        for b in range(1, B):
            assert np.array_equal(a[b], a[0]), (k, b)


# ---- 4. arguments --------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_on_a_live_handle(model):
    """HIPNLP_E_INVALID before anything is launched; the destinations stay as they were"""
    import torch
    from hippopt_amd import _abi
    from hippopt_amd.hipnlp import HipNlpError
    c = case_of(model, "default")
    e, d = c.emu, c.syn
    top, bottom = c.rhs(d, 1)
    t = {k: dev(a) for k, a in dict(hess=d["hess"], jac=d["jac"], top=top, bottom=bottom).items()}
    out = dict(inertia=Guarded((B, 3), integer=True), status=Guarded((B,), integer=True), top=Guarded((B, 1, e.n)), bottom=Guarded((B, 1, e.m)), factor=Guarded((B, e.doubles)),
               pivots=Guarded((B, e.N), integer=True))
    good = dict(nrhs=1, rhs_top_ptr=ptr(t["top"]), rhs_bottom_ptr=ptr(t["bottom"]), sol_top_ptr=out["top"].ptr(), sol_bottom_ptr=out["bottom"].ptr(), stream=_stream())
    pos = [ptr(t["hess"]), ptr(t["jac"]), out["inertia"].ptr(), out["status"].ptr()]

    def refused(call):
        with pytest.raises(HipNlpError) as err:
            call()
        assert err.value.code == _abi.E_INVALID, err.value

    for i in range(4):
        refused(lambda: c.eng.kkt_ldl_device(*(pos[:i] + [0] + pos[i + 1:]), **good))
    for k in ("rhs_top_ptr", "rhs_bottom_ptr", "sol_top_ptr", "sol_bottom_ptr"):
        refused(lambda: c.eng.kkt_ldl_device(*pos, **dict(good, **{k: 0})))
    for kw in (dict(nrhs=-1), dict(nrhs=9), dict(factor_ptr=out["factor"].ptr()), dict(pivots_ptr=out["pivots"].ptr()), dict(max_tries=-1), dict(max_tries=17),
               dict(max_tries=1, delta_init=0.0, kappa=8.0), dict(max_tries=1, delta_init=float("nan"), kappa=8.0), dict(max_tries=1, delta_init=float("inf"), kappa=8.0),
               dict(max_tries=1, delta_init=1e-4, kappa=1.0), dict(max_tries=1, delta_init=1e-4, kappa=float("inf")), dict(max_tries=1, delta_init=1e-4, kappa=float("nan"))):
        refused(lambda: c.eng.kkt_ldl_device(*pos, **dict(good, **kw)))
    sv = [out["factor"].ptr(), out["pivots"].ptr(), 1, ptr(t["top"]), ptr(t["bottom"]), out["top"].ptr(), out["bottom"].ptr()]
    for i in (0, 1, 3, 4, 5, 6):
        refused(lambda: c.eng.kkt_ldl_solve_device(*(sv[:i] + [0] + sv[i + 1:]), stream=_stream()))
    for nrhs in (0, 9):
        refused(lambda: c.eng.kkt_ldl_solve_device(*(sv[:2] + [nrhs] + sv[3:]), stream=_stream()))
    torch.cuda.synchronize()
    assert np.all(np.isnan(out["top"].get())) and np.all(np.isnan(out["bottom"].get())) and np.all(np.isnan(out["factor"].get()))
    assert np.all(out["inertia"].get() == -99) and np.all(out["status"].get() == -99) and np.all(out["pivots"].get() == -99)
    c.eng.kkt_ldl_device(*pos, **dict(good, max_tries=16, delta_init=1e-300, kappa=1.0000001))            # the limits themselves are valid
    torch.cuda.synchronize()
    assert np.all(out["status"].get() >= 0)


# ---- 5. torch ------------------------------------------------------------------------------------------------------------------------------
def test_pose_kkt_values_factor_solve_refine_and_solve_direct(model):
    """PoseKKTValues.factor().solve(refine=1) and solve_direct against the dense numpy solution within the bound of pose_ldl_check; the
    inertia against eigvalsh; the raw calls' bits; a ladder's refinement runs against dx + delta"""
    import torch
    from hippopt_amd.autograd import PoseKKTFactor, PoseNLP
    name = "hands_steps"
    c = case_of(model, name)
    e, st = c.emu, variants(model)[name]
    _, p = ppc.workload(name, st, model, pkc.WORKLOAD_SEED)
    nlp = PoseNLP(st, model, batch=B)
    nlp.set_params(p)
    d = c.real
    dx, dc, bt, bb = (dev(d[k]) for k in ("dx", "dc", "bt", "bb"))
    K = nlp.kkt(dev(c.x), dev(c.sigma), dev(c.lam), dx, dc)
    F = K.factor()
    assert isinstance(F, PoseKKTFactor) and F.factor.shape == (B, e.doubles) and F.pivots.shape == (B, e.N)
    top, bottom = c.rhs(d, 1)
    raw = c.factor(d, d["dx"], d["dc"], top, bottom)
    assert np.array_equal(bits(F.factor.cpu().numpy()), bits(raw["factor"])) and np.array_equal(F.pivots.cpu().numpy(), raw["pivots"])
    assert np.array_equal(F.inertia.cpu().numpy(), raw["inertia"]) and np.all(F.status.cpu().numpy() == 0) and np.all(F.tries.cpu().numpy() == 0)
    z0 = F.solve(bt, bb)
    assert np.array_equal(bits(z0[0].cpu().numpy()), bits(raw["top"][:, 0])) and np.array_equal(bits(z0[1].cpu().numpy()), bits(raw["bottom"][:, 0]))
    z1 = F.solve(bt, bb, refine=1)
    zd = K.solve_direct(bt, bb)
    assert torch.equal(zd[0], z0[0]) and torch.equal(zd[1], z0[1]) and torch.equal(zd[2], F.inertia) and torch.equal(zd[3], F.status)
    z3 = F.solve(dev(c.rhs(d, 3)[0]), dev(c.rhs(d, 3)[1]), refine=1)
    for b in range(B):
        one = {k: a[b] for k, a in d.items()}
        Kd, rhs = plc.dense_of(e, c.pat, one), plc.rhs_of(one)
        bound, ref = plc.eta_bound(Kd, rhs)
        counts, gap = plc.sign_counts(Kd)
        assert gap > 1e-8 and tuple(F.inertia[b].cpu().numpy()) == counts
        for label, z in (("solve", z0), ("refine=1", z1), ("solve_direct", zd), ("nrhs 3, refine=1", (z3[0][:, 0], z3[1][:, 0]))):
            got = plc.eta(Kd, np.concatenate([z[0][b].cpu().numpy(), z[1][b].cpu().numpy()]), rhs)
            print("pose %d %s: eta %.3e, numpy's %.3e, bound %.3e" % (b, label, got, ref, bound))
            assert got <= bound, (b, label)
    # a ladder: the factor is that of dx + delta, and so is the operator the refinement runs against
    Ki = K.with_diagonals(-dx, dc)
    Fi = Ki.factor(**LADDER)
    zi = Fi.solve(bt, bb, refine=1)
    delta = Fi.delta.cpu().numpy()
    assert np.all(Fi.status.cpu().numpy() == 0) and np.all(delta > 0) and np.all(Fi.tries.cpu().numpy() >= 1)
    for b in range(B):
        one = dict({k: a[b] for k, a in d.items()}, dx=-d["dx"][b])
        Kd, rhs = plc.dense_of(e, c.pat, one, delta=float(delta[b])), plc.rhs_of(one)
        assert tuple(Fi.inertia[b].cpu().numpy()) == (e.n, e.m, 0)
        assert plc.eta(Kd, np.concatenate([zi[0][b].cpu().numpy(), zi[1][b].cpu().numpy()]), rhs) <= plc.eta_bound(Kd, rhs)[0], b
