"""GPU: the torch layer of hippopt_amd.autograd under torch.cuda.graph (DESIGN.md "Graph capture").  Every method classified REPLAYABLE
is warmed by one eager call, captured on ONE stream over static tensors and replayed: with input set A, with set B copied into the same
tensors (B is A rolled by one along the batch axis: every batch position sees other data, and in a solve the trajectory that converged
early and the one with iteration 0 land where the first replay ran to the end, and the reverse), once more, and after an eager call of
the same method with other tensors on the same handle (which advances the handle's launch numbers and, for a solve, reuses the MINRES
workspace).  After every replay every output equals, bit for bit, BOTH the eager call's output and the CPU emulation of the kernels
(tests/*_emu_lib.py) — the emulation keeps `both wrong` from passing.  Before any replay the emulation's outputs for A and B are shown to
differ at every batch position, so that no replay can pass by returning what it returned before.  Solves use the conditioned synthetic
Inputs of tests/test_gpu_kkt_minres.py, factor launches the real value runs of tests/test_gpu_kkt_condensed.py (its recipe, on this module's
own handle), the pose finder the real value runs of tests/test_gpu_pose_kkt.py (likewise).  What is classified NOT replayable is refused inside a capture (RuntimeError), the capture ends
normally, the graph is never replayed, and the handle then evaluates eagerly with the bits it gave before.  The backward passes are refused where
their forward pass ran on the capturing stream (autograd runs a backward node on its forward pass's stream): forward eagerly on a stream,
capture on that stream, backward inside — still one stream."""
import numpy as np
import pytest

from test_lagrangian_grad_hostemu import MAKERS

pytestmark = pytest.mark.gpu
B = 3
NXK = 189
FLOOR = 1e-10
RTOL, MAXITER = 1e-8, 100
LADDER = dict(delta_init=1e-4, kappa=8.0, max_tries=8)          # of the pose finder's factorisations
CASES = [("periodic", 3, False), ("stairs", 3, False), ("periodic", 3, True)]      # (name, horizon, lifted)
SOLVES = ["identity", "diagonal", "block", "condensed"]
SYNTHETIC = ["HessianValues.matvec", "JacobianValues.matvec", "JacobianValues.grad_dot", "JacobianValues.jvp", "JacobianValues.rmatvec", "KKTValues.matvec",
             "KKTValues.diagonal_preconditioner"]
FACTORS = ["KKTValues.block_preconditioner", "KKTBlockPreconditioner.apply", "KKTValues.convexify", "KKTValues.condensed_preconditioner", "chain"]
POSE = ["PoseKKTValues.matvec", "PoseKKTValues.diagonal_preconditioner", "PoseKKTValues.solve identity", "PoseKKTValues.solve pair", "PoseKKTValues.solve diagonal",
        "PoseKKTValues.factor", "PoseKKTValues.solve_direct", "PoseKKTFactor.solve", "PoseKKTFactor.solve refined"]
_REFS, _CTX, _POSE = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _nothing_of_this_module_outlives_it():
    """The handles, value runs and emulations this module computes once (its own: _REFS, _CTX, _POSE) go when its last test has run.
    No failure of a later test is known to need this; it keeps four engine handles with their streams, pinned blocks and MINRES
    workspaces from staying alive for the rest of the session only because this module cached them."""
    yield
    import gc
    for cache in (_REFS, _CTX, _POSE):
        cache.clear()
    gc.collect()                                                   # (hipnlp_destroy / hipnlp_pose_destroy of the handles nobody holds any more)


# ---- bytes, input sets ------------------------------------------------------------------------------------------------------------------------------
def raw(a):
    """[batch, bytes] of an array or a tensor"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def rolled(arrays, k):
    return {n: np.roll(a, k, axis=0) for n, a in arrays.items()}


def rows(fn):
    """the outputs of a per-trajectory reference, stacked over the batch: fn(b) -> tuple of arrays or numbers"""
    per = [fn(b) for b in range(B)]
    return [np.stack([np.asarray(p[j]) for p in per]) for j in range(len(per[0]))]


def i32(v):
    return np.asarray(v, dtype=np.int32)


def same_somewhere(ref_a, ref_b, which):
    """[(output, batch position)] at which the two references have the same bytes"""
    return [(j, b) for j in which for b in range(B) if np.array_equal(raw(ref_a[j])[b], raw(ref_b[j])[b])]


# ---- the emulation's references (no device needed) --------------------------------------------------------------------------------------------------
class Refs:
    """the emulations of one layout and the synthetic input set A of its solves and products (tests/test_gpu_kkt_minres.py's Inputs, with
    a grad f run and a sigma for the Jacobian products)"""

    def __init__(self, model, name, horizon, lifted, inputs):
        from hvp_emu_lib import HvpEmu
        from jprod_emu_lib import JprodEmu
        from kkt_condensed_emu_lib import KktCondensedEmu
        from kkt_ladder_emu_lib import KktLadderEmu
        st = MAKERS[name](horizon, model)
        self.emu = KktCondensedEmu(st, model, detect_simple_bounds=lifted)     # ... and the block, diagonal, solve and operator emulations
        self.ladder = KktLadderEmu(st, model, detect_simple_bounds=lifted)
        self.jp, self.hv = JprodEmu(st, model, detect_simple_bounds=lifted), HvpEmu(st, model, detect_simple_bounds=lifted)
        self.n, self.m, self.N = self.emu.n, self.emu.m, horizon
        inp = inputs(self.emu, 100 + horizon)
        self.syn = {k: getattr(inp, k) for k in ("hess", "jac", "dx", "dc", "bt", "bb", "mt", "mb")}
        rng = np.random.RandomState(4100 + horizon)
        self.syn["grad"], self.syn["sigma"] = rng.standard_normal((B, self.n)), rng.uniform(0.2, 2.0, B)

    # -- products and the diagonal on stored value runs
    def product(self, what, S):
        e, jp, hv = self.emu, self.jp, self.hv
        if what == "HessianValues.matvec":
            return rows(lambda b: (hv.hess_times(S["hess"][b], S["bt"][b])[0],))
        if what == "JacobianValues.matvec":
            return rows(lambda b: (jp.jac_times(S["jac"][b], S["bt"][b])[0],))
        if what == "JacobianValues.grad_dot":
            return rows(lambda b: (jp.jac_times(S["jac"][b], S["bt"][b], grad=S["grad"][b], want_jv=False)[1],))
        if what == "JacobianValues.jvp":
            return rows(lambda b: jp.jac_times(S["jac"][b], S["bt"][b], grad=S["grad"][b])[1::-1])
        if what == "JacobianValues.rmatvec":
            return rows(lambda b: (jp.jac_transpose_times(S["jac"][b], S["bb"][b], sigma=S["sigma"][b], grad=S["grad"][b])[0],))
        if what == "KKTValues.matvec":
            return rows(lambda b: e.kkt_times(S["hess"][b], S["jac"][b], S["bt"][b], S["bb"][b], dx=S["dx"][b], dc=S["dc"][b])[:2])
        assert what == "KKTValues.diagonal_preconditioner"
        return rows(lambda b: e.diagonal_preconditioner(S["hess"][b], S["jac"][b], S["dx"][b], S["dc"][b], FLOOR)[:2])

    # -- the preconditioners' records: (factor, pivot words, e, o, inertia, status, top diagonal, bottom)
    def block(self, S, b):
        blk = self.emu.block_factor(S["hess"][b], S["dx"][b], FLOOR)
        diag = self.emu.diagonal_preconditioner(S["hess"][b], S["jac"][b], S["dx"][b], S["dc"][b], FLOOR)
        return blk, (diag.top, diag.bottom)

    def condensed(self, S, b):
        c = self.emu.condensed_factor(S["hess"][b], S["jac"][b], S["dc"][b], S["dx"][b], FLOOR)
        return c, (c.top, c.bottom)

    @staticmethod
    def eight(blk, minv):
        return (blk.factor, i32(blk.words), blk.e, blk.o, i32(blk.inertia), i32(blk.status), minv[0], minv[1])

    @staticmethod
    def five(sol):
        return (sol.top, sol.bottom, i32(sol.iterations), np.float64(sol.residual), i32(sol.status))

    def solve(self, kind, S):
        e = self.emu

        def one(b):
            a = (S["hess"][b], S["jac"][b], S["bt"][b], S["bb"][b])
            if kind in ("identity", "diagonal"):
                return self.five(e.solve(*a, dx=S["dx"][b], dc=S["dc"][b], minv=(S["mt"][b], S["mb"][b]) if kind == "diagonal" else None, rtol=RTOL, maxiter=MAXITER))
            blk, minv = self.block(S, b) if kind == "block" else self.condensed(S, b)
            return self.five(e.block_solve(*a, blk, minv, dx=S["dx"][b], dc=S["dc"][b], rtol=RTOL, maxiter=MAXITER))
        return rows(one)

    def factor(self, what, S):
        e = self.emu

        def one(b):
            if what == "KKTValues.block_preconditioner":
                return self.eight(*self.block(S, b))
            if what == "KKTBlockPreconditioner.apply":
                blk, minv = self.block(S, b)
                return e.block_apply(blk, minv, S["bt"][b], S["bb"][b])[:2]
            if what == "KKTValues.convexify":
                lad = self.ladder.block_ladder(S["hess"][b], S["dx"][b], FLOOR, 1e-4, 8.0, 16)
                dxp = self.ladder.convexified_dx(S["dx"][b], lad.delta)
                diag = e.diagonal_preconditioner(S["hess"][b], S["jac"][b], dxp, S["dc"][b], FLOOR)
                quasi = bool(np.all(lad.status == 0) and np.all(lad.inertia == np.array([NXK, 0, 0])) and np.all(dxp[NXK * self.N:] > 0.0) and np.all(S["dc"][b] > 0.0))
                return self.eight(lad, (diag.top, diag.bottom)) + (lad.delta, i32(lad.tries), np.bool_(quasi), dxp)
            c, minv = self.condensed(S, b)
            if what == "KKTValues.condensed_preconditioner":
                return self.eight(c, minv)
            assert what == "chain"
            sol = e.block_solve(S["hess"][b], S["jac"][b], S["bt"][b], S["bb"][b], c, minv, dx=S["dx"][b], dc=S["dc"][b], rtol=RTOL, maxiter=MAXITER)
            return self.eight(c, minv) + self.five(sol)
        return rows(one)


def refs_of(model, name, horizon, lifted, inputs=None):
    key = (name, horizon, lifted)
    if key not in _REFS:
        if inputs is None:
            from test_gpu_kkt_minres import Inputs as inputs
        _REFS[key] = Refs(model, name, horizon, lifted, inputs)
    return _REFS[key]


# ---- the protocol -----------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


class Slot:
    """the device tensors of one input set, and what is derived from them eagerly (a preconditioner, a factor): load() fills the SAME
    tensors with another set and the derived object's tensors with what it derives from that"""

    def __init__(self, arrays, derive=None):
        self.t = {n: dev(a) for n, a in arrays.items()}
        self.derive = derive
        self.d, self.dt = derive(self.t) if derive else (None, [])

    def load(self, arrays):
        import torch
        for n, a in arrays.items():
            self.t[n].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        if self.derive:
            for old, new in zip(self.dt, self.derive(self.t)[1]):
                old.copy_(new)


def record(pre):
    return [pre.factor, pre.pivots, pre.e, pre.o, pre.inertia, pre.status, pre.top_diagonal, pre.bottom]


def protocol(what, A, call, reference, derive=None, floats=None, then=()):
    """call(slot) -> the output tensors; reference(set) -> the emulation's outputs [batch, ...]; floats: the outputs that must differ
    between A and B at every batch position (default: all); then: [(label, set, nan_in_trajectory_0)] replayed after the protocol"""
    import torch
    Bs, Cs = rolled(A, 1), rolled(A, 2)
    ref_a, ref_b = reference(A), reference(Bs)
    same = same_somewhere(ref_a, ref_b, range(len(ref_a)) if floats is None else floats)
    assert not same, (what, "the emulation expects the same bytes from A and B at (output, batch position)", same)

    def check(outs, refs, where, nan_aware=False):
        torch.cuda.synchronize()
        assert len(outs) == len(refs), (what, where)
        for j, (o, r) in enumerate(zip(outs, refs)):
            got, want = raw(o), raw(r)
            assert got.shape == want.shape, (what, where, "output %d" % j, got.shape, want.shape)
            if nan_aware and np.asarray(r).dtype == np.float64:
                o = o.cpu().numpy()
                bad = [b for b in range(B) if not np.array_equal(o[b], np.asarray(r)[b], equal_nan=True) or (b > 0 and not np.array_equal(got[b], want[b]))]
            else:
                bad = [b for b in range(B) if not np.array_equal(got[b], want[b])]
            assert not bad, (what, where, "output %d differs at the batch positions" % j, bad)

    static, other = Slot(A, derive), Slot(Cs, derive)
    eager_a = [o.clone() for o in call(static)]                    # 1. warm: eagerly, A then B
    check(eager_a, ref_a, "eager, A")
    static.load(Bs)
    eager_b = [o.clone() for o in call(static)]
    check(eager_b, ref_b, "eager, B")
    static.load(A)                                                 # 2. static tensors hold A
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # 3. one stream: torch.cuda.graph's own
        outs = list(call(static))
    graph.replay()                                                 # 4.
    check(outs, ref_a, "first replay, A")
    check(outs, eager_a, "first replay, A, against the eager call")
    static.load(Bs)                                                # 5.
    graph.replay()
    check(outs, ref_b, "replay, B")
    check(outs, eager_b, "replay, B, against the eager call")
    graph.replay()                                                 # 6.
    check(outs, ref_b, "second replay, B")
    call(other)                                                    # 7. eagerly, other tensors, the same handle
    graph.replay()                                                 # 8.
    check(outs, ref_b, "replay after an eager call on the handle, B")
    for label, S, nan_in_0 in then:
        static.load(S)
        eager = [o.clone() for o in call(static)]
        graph.replay()
        check(outs, reference(S), label, nan_aware=nan_in_0)
        check(outs, eager, label + ", against the eager call")
    return graph


# ---- the kinodynamic NLP ----------------------------------------------------------------------------------------------------------------------------
def ctx_of(model, name, horizon, lifted):
    """(references, nlp, the real input set A), computed once on a handle of this module's own.  The value runs are those of real() of
    tests/test_gpu_kkt_condensed.py, by its recipe: the KKT system of the synthetic workload's iterate (seed 8900, the stairs' first
    trajectory on the flanks), sigma 0.8, RandomState(11) for lambda, dx, dc in U[1, 2] and the right-hand side, on the device's own runs"""
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    from hippopt_amd.synthetic import make_workload, place_on_step_flanks
    key = (name, horizon, lifted)
    if key not in _CTX:
        st = MAKERS[name](horizon, model)
        x, p = make_workload(st, model, batch=B, seed=8900)
        if name == "stairs":
            place_on_step_flanks(x[:1], st, seed=3)
        nlp = KinodynamicNLP(st, model, batch=B, detect_simple_bounds=lifted)
        nlp.set_params(p)
        rng = np.random.RandomState(11)
        lam, dx, dc = rng.standard_normal((B, nlp.m)), rng.uniform(1.0, 2.0, (B, nlp.n)), rng.uniform(1.0, 2.0, (B, nlp.m))
        d = dict(dx=dx, dc=dc, bt=rng.standard_normal((B, nlp.n)), bb=rng.standard_normal((B, nlp.m)))
        K = nlp.kkt(dev(x), 0.8, dev(lam), dev(dx), dev(dc))
        torch.cuda.synchronize()
        d["hess"], d["jac"] = K.hess.cpu().numpy(), K.jac.cpu().numpy()
        assert np.all(np.isfinite(d["hess"])) and np.all(np.isfinite(d["jac"]))
        _CTX[key] = (refs_of(model, name, horizon, lifted), nlp, d, x, p)
    return _CTX[key][:3]


def workload_of(model, name, horizon, lifted):
    """(x, p) of ctx_of's handle"""
    ctx_of(model, name, horizon, lifted)
    return _CTX[(name, horizon, lifted)][3:]


def kkt(nlp, t):
    from hippopt_amd.autograd import KKTValues
    return KKTValues(nlp, t["hess"], t["jac"], t["dx"], t["dc"])


@pytest.mark.parametrize("what", SYNTHETIC)
@pytest.mark.parametrize("name,horizon,lifted", CASES)
def test_products_on_stored_value_runs_replay(model, name, horizon, lifted, what):
    from hippopt_amd.autograd import HessianValues, JacobianValues
    r, nlp, _ = ctx_of(model, name, horizon, lifted)
    J = lambda t: JacobianValues(nlp, t["grad"], t["jac"])  # noqa: E731
    calls = {
        "HessianValues.matvec": lambda s: (HessianValues(nlp, s.t["hess"]).matvec(s.t["bt"]),),
        "JacobianValues.matvec": lambda s: (J(s.t).matvec(s.t["bt"]),),
        "JacobianValues.grad_dot": lambda s: (J(s.t).grad_dot(s.t["bt"]),),
        "JacobianValues.jvp": lambda s: J(s.t).jvp(s.t["bt"]),
        "JacobianValues.rmatvec": lambda s: (J(s.t).rmatvec(s.t["sigma"], s.t["bb"]),),
        "KKTValues.matvec": lambda s: kkt(nlp, s.t).matvec(s.t["bt"], s.t["bb"]),
        "KKTValues.diagonal_preconditioner": lambda s: kkt(nlp, s.t).diagonal_preconditioner(FLOOR),
    }
    protocol("%s %s N=%d lifted=%s" % (what, name, horizon, lifted), r.syn, calls[what], lambda S: r.product(what, S))


@pytest.mark.parametrize("kind", SOLVES)
@pytest.mark.parametrize("name,horizon,lifted", CASES)
def test_solves_replay_from_a_clean_start(model, name, horizon, lifted, kind):
    """check_every=0, maxiter 100.  In A trajectory 1 converges before trajectory 0 and trajectory 2 (b = 0) has iteration 0 and status 0;
    B puts each of them where another ran in the replay before.  After the protocol: a set whose trajectory 0 has a NaN in its right-hand
    side (status 2: breakdown), then A again — a breakdown record must not survive into the next replay.  (Of the NaN set, the emulation
    fixes status, iterations and which elements are NaN; the bits of a NaN are left to the eager call on the device: IEEE 754 does not
    fix the sign and payload an operation gives a NaN, and the host's and the device's arithmetic differ in them.)"""
    r, nlp, _ = ctx_of(model, name, horizon, lifted)
    ref = r.solve(kind, r.syn)
    its, status = ref[2].tolist(), ref[4].tolist()
    print("%s N=%d lifted=%s %s: the emulation's iterations %s, status %s" % (name, horizon, lifted, kind, its, status))
    assert status[2] == 0 and its[2] == 0 and its[0] > 0 and its[1] > 0
    assert kind != "identity" or (status[:2] == [0, 0] and its[1] < its[0] < MAXITER)      # (the other kinds: whatever the emulation says)
    derive = None
    if kind in ("block", "condensed"):
        def derive(t):
            pre = kkt(nlp, t).block_preconditioner(FLOOR) if kind == "block" else kkt(nlp, t).condensed_preconditioner(FLOOR)
            return pre, [pre.factor, pre.pivots, pre.e, pre.o, pre.top_diagonal, pre.bottom]

    def call(s):
        minv = s.d if derive else (s.t["mt"], s.t["mb"]) if kind == "diagonal" else None
        return tuple((s.d.values if derive else kkt(nlp, s.t)).solve(s.t["bt"], s.t["bb"], rtol=RTOL, maxiter=MAXITER, minv=minv, check_every=0))
    nan = {k: a.copy() for k, a in r.syn.items()}
    nan["bt"][0, 3] = np.nan
    broken = r.solve(kind, nan)
    assert broken[4].tolist() == [2, status[1], status[2]], broken[4]
    protocol("solve %s %s N=%d lifted=%s" % (kind, name, horizon, lifted), r.syn, call, lambda S: r.solve(kind, S), derive, floats=(0, 1, 3),
             then=[("a NaN in trajectory 0", nan, True), ("A again, after the breakdown", r.syn, False)])


@pytest.mark.parametrize("what", FACTORS)
@pytest.mark.parametrize("name,horizon,lifted", CASES)
def test_factor_launches_and_the_chain_replay(model, name, horizon, lifted, what):
    """on the real value runs; convexify is captured whole, with its torch operations between the two launches; `chain` is
    condensed_preconditioner -> solve(minv=pre, check_every=0) in ONE graph"""
    r, nlp, real = ctx_of(model, name, horizon, lifted)
    derive = None
    if what == "KKTBlockPreconditioner.apply":
        def derive(t):
            pre = kkt(nlp, t).block_preconditioner(FLOOR)
            return pre, [pre.factor, pre.pivots, pre.e, pre.o, pre.top_diagonal, pre.bottom]

    def chain(s):
        K = kkt(nlp, s.t)
        pre = K.condensed_preconditioner(FLOOR)
        return tuple(record(pre)) + tuple(K.solve(s.t["bt"], s.t["bb"], rtol=RTOL, maxiter=MAXITER, minv=pre, check_every=0))

    def convexify(s):
        pre = kkt(nlp, s.t).convexify(1e-4, 8.0, 16, FLOOR)
        return tuple(record(pre)) + (pre.delta, pre.tries, pre.quasi_definite, pre.values.dx)
    calls = {
        "KKTValues.block_preconditioner": lambda s: tuple(record(kkt(nlp, s.t).block_preconditioner(FLOOR))),
        "KKTBlockPreconditioner.apply": lambda s: s.d.apply(s.t["bt"], s.t["bb"]),
        "KKTValues.convexify": convexify,
        "KKTValues.condensed_preconditioner": lambda s: tuple(record(kkt(nlp, s.t).condensed_preconditioner(FLOOR))),
        "chain": chain,
    }
    # (factor, e, the two diagonals, and what follows them; not o, which is zero wherever every pivot is 1 x 1, nor the integers)
    floats = {"KKTValues.convexify": (0, 2, 6, 7, 11), "chain": (0, 2, 6, 7, 8, 9, 11)}.get(what, (0, 1) if derive else (0, 2, 6, 7))
    protocol("%s %s N=%d lifted=%s" % (what, name, horizon, lifted), real, calls[what], lambda S: r.factor(what, S), derive, floats=floats)


# ---- what is refused ----------------------------------------------------------------------------------------------------------------------------------
def refused(call, match, stream=None):
    """the call inside a capture (on `stream`: torch.cuda.graph's own when None) that also holds one torch operation: RuntimeError, and
    the capture ends normally; never replayed"""
    import torch
    one = torch.ones(4, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        two = one + one
        with pytest.raises(RuntimeError, match=match):
            call()
    torch.cuda.synchronize()
    del two, graph


@pytest.mark.parametrize("name,horizon,lifted", CASES[:2])
def test_what_is_not_replayable_is_refused_in_a_capture_and_the_handle_is_as_before(model, name, horizon, lifted):
    """after EVERY refusal the handle evaluates eagerly with the bits it gave before.  The backward passes: autograd runs a backward node
    on the stream of its forward pass, so the guard sees a capture only where the forward pass ran on the capturing stream — that case
    is tested here, on ONE stream: forward eagerly on s, capture on s, backward inside.  (A forward pass on another stream is torch's
    and the runtime's to refuse: the engine would have to join a stream that is not capturing to one that is.)"""
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    r, nlp, real = ctx_of(model, name, horizon, lifted)
    st = MAKERS[name](horizon, model)
    xh, p = workload_of(model, name, horizon, lifted)
    x, lam, v, sigma = dev(xh), dev(real["bb"]), dev(real["bt"]), dev(r.syn["sigma"])
    t = {k: dev(a) for k, a in real.items()}
    K = kkt(nlp, t)

    def everything():
        f, g = nlp(x)
        J = nlp.jacobian(x)
        z = K.solve(t["bt"], t["bb"], maxiter=20, check_every=5)
        outs = [f, g, J.grad, J.values, nlp.lagrangian_gradient(x, sigma, lam), nlp.hessian_vector_product(x, sigma, lam, v), nlp.hessian(x, sigma, lam).values,
                *nlp.jacobian_vector_product(x, v), nlp.kkt(x, sigma, lam).hess, *z]
        torch.cuda.synchronize()
        return [raw(o).copy() for o in outs]
    before = everything()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                     # the forward passes eagerly, on the stream that will capture
        xg = x.clone().requires_grad_()
        f, g = nlp(xg)
        gx = nlp.lagrangian_gradient(xg, sigma, lam)               # recorded: its backward pass is the Hessian-vector product
    torch.cuda.synchronize()
    for call, match, stream in ((lambda: (f.sum() + g.sum()).backward(retain_graph=True), "backward pass of nlp.x. cannot be captured", s),
                                (lambda: gx.sum().backward(retain_graph=True), "double backward pass of nlp.x. cannot be captured", s)):
        refused(call, match, stream)
        assert xg.grad is None
        assert all(np.array_equal(a, b) for a, b in zip(before, everything())), match
    (f.sum() + g.sum()).backward()                                 # ... and outside the capture the recorded graph is whole
    torch.cuda.synchronize()
    assert np.array_equal(raw(xg.grad), raw(nlp.lagrangian_gradient(x, 1.0, torch.ones_like(lam))))
    for call, match in ((lambda: nlp(x), "KinodynamicNLP.__call__.*launch number"),
                        (lambda: nlp.jacobian(x), "KinodynamicNLP.jacobian cannot be captured"),
                        (lambda: nlp.jacobian_vector_product(x, v), "KinodynamicNLP.jacobian_vector_product cannot be captured"),
                        (lambda: nlp.kkt(x, sigma, lam), "KinodynamicNLP.kkt cannot be captured"),
                        (lambda: nlp.lagrangian_gradient(x, sigma, lam), "KinodynamicNLP.lagrangian_gradient cannot be captured"),
                        (lambda: nlp.hessian_vector_product(x, sigma, lam, v), "KinodynamicNLP.hessian_vector_product cannot be captured"),
                        (lambda: nlp.hessian(x, sigma, lam), "KinodynamicNLP.hessian cannot be captured"),
                        (lambda: nlp.set_params(p), "set_params cannot be captured"),
                        (lambda: K.solve(t["bt"], t["bb"], maxiter=20, check_every=5), "check_every=0")):
        refused(call, match)
        after = everything()
        assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after)), match
    # a first use: J.jvp after only J.matvec was warmed, on a handle of its own
    fresh = KinodynamicNLP(st, model, batch=B, detect_simple_bounds=lifted)
    fresh.set_params(p)
    J = fresh.jacobian(x)
    jv = J.matvec(v)
    refused(lambda: J.jvp(v), "JacobianValues.jvp: first use.*once outside the capture")
    refused(lambda: J.grad_dot(v), "JacobianValues.grad_dot: first use.*once outside the capture")
    dot, jv2 = J.jvp(v)
    torch.cuda.synchronize()
    assert np.array_equal(raw(jv), raw(jv2)) and np.array_equal(raw(jv), raw(J.matvec(v)))
    want = rows(lambda b: r.jp.jac_times(J.values[b].cpu().numpy(), real["bt"][b], grad=J.grad[b].cpu().numpy())[1::-1])
    assert np.array_equal(raw(dot), raw(want[0])) and np.array_equal(raw(jv2), raw(want[1]))


# ---- the pose finder ----------------------------------------------------------------------------------------------------------------------------------
def pose_ctx(model):
    """(nlp, the KKT emulation, the L D L^T emulation, the real input set A), on a handle of this module's own: by the recipe of the
    `default` case of tests/test_gpu_pose_kkt.py — the device's own value runs at the three poses of the workload, the diagonals and
    right-hand sides of pose_kkt_check.inputs"""
    if not _POSE:
        import torch
        import pose_kkt_check as pkc
        import pose_products_check as ppc
        from hippopt_amd.autograd import PoseNLP
        from pose_kkt_emu_lib import PoseKktEmu
        from pose_ldl_emu_lib import PoseLdlEmu
        from test_pose_body_hostemu import variants
        st = variants(model)["default"]
        ke = PoseKktEmu(st, model)
        nlp = PoseNLP(st, model, batch=B)
        x, p = ppc.workload("default", st, model, pkc.WORKLOAD_SEED)
        nlp.set_params(p)
        lam, sigma, _ = ppc.factors(ke.m, ke.n, pkc.FACTOR_SEED)
        syn, real = pkc.inputs(ke.n, ke.m, ke.nnz, ke.hnnz)
        d = {k: np.stack([real[b][k] for b in range(B)]) for k in ("dx", "dc", "bt", "bb")}
        d["mt"], d["mb"] = (np.stack([syn[0][k], syn[1][k], syn[0][k]]) for k in ("mt", "mb"))
        K = nlp.kkt(dev(x), dev(sigma), dev(lam))
        torch.cuda.synchronize()
        d["hess"], d["jac"] = K.hess.cpu().numpy(), K.jac.cpu().numpy()
        assert np.all(np.isfinite(d["hess"])) and np.all(np.isfinite(d["jac"]))
        _POSE["ctx"] = (nlp, ke, PoseLdlEmu(st, model), d)
    return _POSE["ctx"]


def pose_reference(what, S, ke, le):
    def one(b):
        runs = (S["hess"][b], S["jac"][b])
        dx, dc, bt, bb = S["dx"][b], S["dc"][b], S["bt"][b], S["bb"][b]
        if what == "PoseKKTValues.matvec":
            return ke.times(*runs, bt, bb, dx, dc)[:2]
        if what == "PoseKKTValues.diagonal_preconditioner":
            return ke.diagonal_preconditioner(*runs, dx, dc, FLOOR)[:2]
        if what.startswith("PoseKKTValues.solve "):
            minv = {"identity": None, "pair": (S["mt"][b], S["mb"][b]), "diagonal": "diagonal"}[what.split(" ")[1]]
            return Refs.five(ke.solve(*runs, bt, bb, dx, dc, minv=minv, floor=FLOOR, rtol=RTOL, maxiter=MAXITER))
        if what == "PoseKKTValues.solve_direct":
            f = le.factor(*runs, dx, dc, bt[None], bb[None], store=False, **LADDER)
            return (f.top[0], f.bottom[0], i32(f.inertia), i32(f.status))
        f = le.factor(*runs, dx, dc, store=True, **LADDER)
        if what == "PoseKKTValues.factor":
            return (f.factor, i32(f.pivots), i32(f.inertia), i32(f.status), np.float64(f.delta), i32(f.tries))
        top, bottom = (a[0] for a in le.solve(f.factor, f.pivots, bt[None], bb[None]))
        if what == "PoseKKTFactor.solve refined":                 # one round: r = b - (K + delta I_top) z, z += solve(r); torch's elementwise IEEE operations
            kt, kb = ke.times(*runs, top, bottom, dx + f.delta, dc)[:2]
            et, eb = (a[0] for a in le.solve(f.factor, f.pivots, (bt - kt)[None], (bb - kb)[None]))
            top, bottom = top + et, bottom + eb
        return (top, bottom)
    return rows(one)


@pytest.mark.parametrize("what", POSE)
def test_the_pose_finders_stored_value_launches_replay(model, what):
    from hippopt_amd.autograd import PoseKKTValues
    nlp, ke, le, real = pose_ctx(model)
    K = lambda t: PoseKKTValues(nlp, t["hess"], t["jac"], t["dx"], t["dc"])  # noqa: E731
    derive = None
    if what.startswith("PoseKKTFactor"):
        def derive(t):
            F = K(t).factor(**LADDER)
            return F, [F.factor, F.pivots, F.delta]

    def solve(s):
        minv = {"identity": None, "pair": (s.t["mt"], s.t["mb"]), "diagonal": "diagonal"}[what.split(" ")[1]]
        return tuple(K(s.t).solve(s.t["bt"], s.t["bb"], rtol=RTOL, maxiter=MAXITER, minv=minv, floor=FLOOR))

    def factor(s):
        F = K(s.t).factor(**LADDER)
        return (F.factor, F.pivots, F.inertia, F.status, F.delta, F.tries)
    calls = {
        "PoseKKTValues.matvec": lambda s: K(s.t).matvec(s.t["bt"], s.t["bb"]),
        "PoseKKTValues.diagonal_preconditioner": lambda s: K(s.t).diagonal_preconditioner(FLOOR),
        "PoseKKTValues.factor": factor,
        "PoseKKTValues.solve_direct": lambda s: K(s.t).solve_direct(s.t["bt"], s.t["bb"], **LADDER),
        "PoseKKTFactor.solve": lambda s: s.d.solve(s.t["bt"], s.t["bb"]),
        "PoseKKTFactor.solve refined": lambda s: s.d.solve(s.t["bt"], s.t["bb"], refine=1),
    }
    floats = (0, 1, 3) if " " in what and what.startswith("PoseKKTValues.solve ") else (0,) if what == "PoseKKTValues.factor" else (0, 1)
    protocol(what, real, calls.get(what, solve), lambda S: pose_reference(what, S, ke, le), derive, floats=floats)


def test_the_pose_finders_evaluations_are_refused_in_a_capture_and_the_handle_is_as_before(model):
    import torch
    import pose_kkt_check as pkc
    import pose_products_check as ppc
    from test_pose_body_hostemu import variants
    nlp, ke, le, real = pose_ctx(model)
    xh, p = ppc.workload("default", variants(model)["default"], model, pkc.WORKLOAD_SEED)
    x, lam, v, sigma = dev(xh), dev(real["bb"]), dev(real["bt"]), dev(np.array([0.7, 1.1, 1.9]))

    def everything():
        f, g = nlp(x)
        K = nlp.kkt(x, sigma, lam)
        outs = [f, g, nlp.lagrangian_gradient(x, sigma, lam), *nlp.jacobian_vector_product(x, v), nlp.hessian_vector_product(x, sigma, lam, v), K.hess, K.jac]
        torch.cuda.synchronize()
        return [raw(o).copy() for o in outs]
    before = everything()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                     # the forward passes eagerly, on the stream that will capture
        xg = x.clone().requires_grad_()
        f, g = nlp(xg)
        gx = nlp.lagrangian_gradient(xg, sigma, lam)
    torch.cuda.synchronize()
    for call, match in ((lambda: (f.sum() + g.sum()).backward(retain_graph=True), "backward pass of nlp.x. cannot be captured"),
                        (lambda: gx.sum().backward(retain_graph=True), "double backward pass of nlp.x. cannot be captured")):
        refused(call, match, s)
        assert xg.grad is None
        assert all(np.array_equal(a, b) for a, b in zip(before, everything())), match
    (f.sum() + g.sum()).backward()
    torch.cuda.synchronize()
    assert np.array_equal(raw(xg.grad), raw(nlp.lagrangian_gradient(x, 1.0, torch.ones_like(lam))))
    for call, method in ((lambda: nlp(x), "PoseNLP.__call__"), (lambda: nlp.lagrangian_gradient(x, sigma, lam), "PoseNLP.lagrangian_gradient"),
                         (lambda: nlp.jacobian_vector_product(x, v), "PoseNLP.jacobian_vector_product"),
                         (lambda: nlp.hessian_vector_product(x, sigma, lam, v), "PoseNLP.hessian_vector_product"), (lambda: nlp.kkt(x, sigma, lam), "PoseNLP.kkt"),
                         (lambda: nlp.set_params(p), "set_params")):
        refused(call, method + " cannot be captured")
        assert all(np.array_equal(a, b) for a, b in zip(before, everything())), method
