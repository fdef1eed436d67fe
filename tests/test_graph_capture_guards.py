"""CPU: the graph-capture guards of hippopt_amd.autograd (DESIGN.md "Graph capture"), on a stub engine that records every call, with
torch.cuda.is_current_stream_capturing patched.  For every guarded path — a method that is not replayable, solve(check_every > 0), a
first-ever use — the RuntimeError comes BEFORE any engine method was called, and names the method and the remedy; a warmed replayable
method asks torch nothing; the side-stream branch of _on_current_stream is never taken while capturing.  What replays correctly is
proved on the device: tests/test_gpu_graph_replay.py."""
import numpy as np
import pytest
import torch

from hippopt_amd import autograd
from hippopt_amd.autograd import KinodynamicNLP, KKTValues, PoseKKTValues, PoseNLP

B, N = 2, 1
NXK = 189


class StubEngine:
    """records (name, args) of every method called on it; nothing else"""

    def __init__(self, **attributes):
        self.calls = []
        self.returns = {}
        self.__dict__.update(attributes)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def method(*args, **kwargs):
            self.calls.append(name)
            return self.returns.get(name)
        return method


class StubKinodynamic(KinodynamicNLP):
    device = torch.device("cpu")

    def __init__(self, jacobian_products=False):
        n, m = NXK * N + 6, 5
        self.engine = StubEngine(batch=B, n=n, m=m, np=3, nnz=11)
        self.engine.returns.update(hess_nnz=13, kkt_block_bytes=(8 * B * N * NXK * (NXK + 1) // 2, 4 * B * N * NXK, 8 * B * N * NXK))
        self.batch, self.n, self.m, self.np, self.device_index, self.jacobian_products = B, n, m, 3, 0, jacobian_products


class StubPose(PoseNLP):
    device = torch.device("cpu")

    def __init__(self):
        self.engine = StubEngine(batch=B, n=81, m=4, np=202, nnz=9)
        self.engine.returns.update(kkt_ldl_doubles=85 * 86 // 2)
        self.batch, self.n, self.m, self.np, self.device_index, self._hess_nnz = B, 81, 4, 202, 0, 17


class Stream:
    def __init__(self, handle):
        self.cuda_stream = handle

    def wait_stream(self, other):
        raise AssertionError("a fork or join of streams")


class Torch:
    """what the test patches into torch.cuda: a stream of the capture's own, and the answer to `is the stream capturing`"""

    def __init__(self, monkeypatch, handle=0x1234):
        self.capturing, self.queries, self.forbid_queries = False, 0, False
        monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: Stream(handle))
        monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: Stream(0x77))
        monkeypatch.setattr(torch.cuda, "is_initialized", lambda: True)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", self.query)

    def query(self):
        assert not self.forbid_queries, "a warmed replayable method asked torch whether the stream is capturing"
        self.queries += 1
        return self.capturing


def t(*shape):
    return torch.zeros(*shape, dtype=torch.float64)


def kinodynamic_values(nlp):
    """(J, H, K) on the stub, built eagerly"""
    J, H = nlp.jacobian(t(B, nlp.n)), nlp.hessian(t(B, nlp.n), 1.0, t(B, nlp.m))
    K = KKTValues(nlp, H, J, t(B, nlp.n), t(B, nlp.m))
    return J, H, K


# every replayable method: name -> (what builds its receiver eagerly WITHOUT warming the method, the call)
def kinodynamic_replayable():
    lam, v, w = (lambda nlp: t(B, nlp.m)), (lambda nlp: t(B, nlp.n)), (lambda nlp: t(B, nlp.m))
    sig = lambda nlp: t(B)  # noqa: E731
    return {
        "HessianValues.matvec": lambda nlp, J, H, K: H.matvec(v(nlp)),
        "JacobianValues.matvec": lambda nlp, J, H, K: J.matvec(v(nlp)),
        "JacobianValues.grad_dot": lambda nlp, J, H, K: J.grad_dot(v(nlp)),
        "JacobianValues.jvp": lambda nlp, J, H, K: J.jvp(v(nlp)),
        "JacobianValues.rmatvec": lambda nlp, J, H, K: J.rmatvec(sig(nlp), lam(nlp)),
        "KKTValues.matvec": lambda nlp, J, H, K: K.matvec(v(nlp), w(nlp)),
        "KKTValues.diagonal_preconditioner": lambda nlp, J, H, K: K.diagonal_preconditioner(),
        "KKTValues.block_preconditioner": lambda nlp, J, H, K: K.block_preconditioner(),
        "KKTValues.convexify": lambda nlp, J, H, K: K.convexify(),
        "KKTValues.condensed_preconditioner": lambda nlp, J, H, K: K.condensed_preconditioner(),
        "KKTValues.solve": lambda nlp, J, H, K: K.solve(v(nlp), w(nlp), check_every=0),
        "KKTValues.solve minv": lambda nlp, J, H, K: K.solve(v(nlp), w(nlp), minv=(v(nlp), w(nlp)), check_every=0),
    }


def pose_replayable():
    x, lam = (lambda: t(B, 81)), (lambda: t(B, 4))
    return {
        "PoseKKTValues.matvec": lambda nlp, K: K.matvec(x(), lam()),
        "PoseKKTValues.diagonal_preconditioner": lambda nlp, K: K.diagonal_preconditioner(),
        "PoseKKTValues.solve": lambda nlp, K: K.solve(x(), lam()),
        "PoseKKTValues.solve diagonal": lambda nlp, K: K.solve(x(), lam(), minv="diagonal"),
        "PoseKKTValues.factor": lambda nlp, K: K.factor(),
        "PoseKKTValues.solve_direct": lambda nlp, K: K.solve_direct(x(), lam()),
    }


def pose_values(nlp):
    return PoseKKTValues(nlp, t(B, nlp.hess_nnz), t(B, nlp.engine.nnz), t(B, 81), t(B, 4))


# ---- 1. first-ever use while capturing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kinodynamic_replayable()))
def test_a_first_use_while_capturing_is_refused_before_any_engine_call(monkeypatch, name):
    tc = Torch(monkeypatch)
    nlp = StubKinodynamic()
    J, H, K = kinodynamic_values(nlp)
    nlp.engine.calls.clear()
    tc.capturing = True
    with pytest.raises(RuntimeError, match="once outside the capture") as err:
        kinodynamic_replayable()[name](nlp, J, H, K)
    assert name.split(" ")[0] in str(err.value) and "first use" in str(err.value)
    assert nlp.engine.calls == []
    tc.capturing = False                                           # ... and nothing was left half-prepared: the eager call runs
    kinodynamic_replayable()[name](nlp, J, H, K)
    assert nlp.engine.calls != []


@pytest.mark.parametrize("name", sorted(pose_replayable()))
def test_a_first_use_of_the_pose_finder_while_capturing_is_refused_before_any_engine_call(monkeypatch, name):
    tc = Torch(monkeypatch)
    nlp = StubPose()
    K = pose_values(nlp)
    tc.capturing = True
    with pytest.raises(RuntimeError, match="once outside the capture") as err:
        pose_replayable()[name](nlp, K)
    assert name.split(" ")[0] in str(err.value)
    assert nlp.engine.calls == []


def test_the_stored_pose_factor_is_guarded_too(monkeypatch):
    tc = Torch(monkeypatch)
    nlp = StubPose()
    F = pose_values(nlp).factor()
    F.solve(t(B, 81), t(B, 4))                                     # warms the solve from the factor, not the matvec of the refinement
    nlp.engine.calls.clear()
    tc.capturing = True
    F.solve(t(B, 81), t(B, 4))
    assert nlp.engine.calls == ["kkt_ldl_solve_device"]
    nlp.engine.calls.clear()
    with pytest.raises(RuntimeError, match="PoseKKTFactor.solve.*kkt_times"):
        F.solve(t(B, 81), t(B, 4), refine=1)
    assert nlp.engine.calls == []                                  # (not even the first solve of the refinement)


def test_jvp_is_not_warmed_by_matvec(monkeypatch):
    """hipnlp_jac_times_device allocates the dot's partials the first time a dot is asked for: J.matvec can have run while J.jvp and
    J.grad_dot still allocate"""
    tc = Torch(monkeypatch)
    nlp = StubKinodynamic()
    J, H, K = kinodynamic_values(nlp)
    J.matvec(t(B, nlp.n))
    nlp.engine.calls.clear()
    tc.capturing = True
    J.matvec(t(B, nlp.n))
    assert nlp.engine.calls == ["jac_times_device"]
    nlp.engine.calls.clear()
    for call in (J.jvp, J.grad_dot):
        with pytest.raises(RuntimeError, match="once outside the capture"):
            call(t(B, nlp.n))
    assert nlp.engine.calls == []
    tc.capturing = False
    J.jvp(t(B, nlp.n))
    tc.capturing = True
    J.jvp(t(B, nlp.n))                                             # warmed now; grad_dot alone is another kind still
    with pytest.raises(RuntimeError, match="JacobianValues.grad_dot"):
        J.grad_dot(t(B, nlp.n))


def test_the_kinds_of_minv_are_warmed_separately_and_belong_to_the_handle(monkeypatch):
    tc = Torch(monkeypatch)
    nlp = StubKinodynamic()
    J, H, K = kinodynamic_values(nlp)
    rhs = t(B, nlp.n), t(B, nlp.m)
    K.solve(*rhs, check_every=0)
    pre = K.block_preconditioner()
    tc.capturing = True
    K.solve(*rhs, check_every=0)
    nlp.engine.calls.clear()
    for minv in (rhs, pre):
        with pytest.raises(RuntimeError, match="KKTValues.solve"):
            K.solve(*rhs, minv=minv, check_every=0)
    with pytest.raises(RuntimeError, match="KKTBlockPreconditioner.apply.*once outside the capture"):
        pre.apply(*rhs)
    assert nlp.engine.calls == []
    nlp.engine = StubEngine(**{k: getattr(nlp.engine, k) for k in ("batch", "n", "m", "np", "nnz")})      # another handle: nothing of it is warm
    with pytest.raises(RuntimeError, match="once outside the capture"):
        K.solve(*rhs, check_every=0)
    assert nlp.engine.calls == []


# ---- 2. what is not replayable ------------------------------------------------------------------------------------------------------------------
def not_replayable():
    x, lam, sig = (lambda nlp: t(B, nlp.n)), (lambda nlp: t(B, nlp.m)), (lambda nlp: t(B))
    return {
        "KinodynamicNLP.lagrangian_gradient": (lambda nlp, J, H, K: nlp.lagrangian_gradient(x(nlp), sig(nlp), lam(nlp)), "outside the capture"),
        "KinodynamicNLP.hessian_vector_product": (lambda nlp, J, H, K: nlp.hessian_vector_product(x(nlp), sig(nlp), lam(nlp), x(nlp)), "outside the capture"),
        "KinodynamicNLP.hessian": (lambda nlp, J, H, K: nlp.hessian(x(nlp), sig(nlp), lam(nlp)), "outside the capture"),
        "KinodynamicNLP.__call__": (lambda nlp, J, H, K: nlp(t(B, nlp.n)), "launch number"),
        "KinodynamicNLP.jacobian": (lambda nlp, J, H, K: nlp.jacobian(t(B, nlp.n)), "outside the capture"),
        "KinodynamicNLP.jacobian_vector_product": (lambda nlp, J, H, K: nlp.jacobian_vector_product(t(B, nlp.n), t(B, nlp.n)), "outside the capture"),
        "KinodynamicNLP.kkt": (lambda nlp, J, H, K: nlp.kkt(t(B, nlp.n), 1.0, t(B, nlp.m)), "outside the capture"),
        "set_params": (lambda nlp, J, H, K: nlp.set_params(np.zeros((B, 3))), "outside the capture"),
        "KKTValues.solve(check_every=5)": (lambda nlp, J, H, K: K.solve(t(B, nlp.n), t(B, nlp.m), check_every=5), "check_every=0"),
        "KKTValues.solve(check_every=16)": (lambda nlp, J, H, K: K.solve(t(B, nlp.n), t(B, nlp.m)), "check_every=0"),
    }


@pytest.mark.parametrize("name", sorted(not_replayable()))
def test_what_is_not_replayable_is_refused_before_any_engine_call_however_warm(monkeypatch, name):
    tc = Torch(monkeypatch)
    nlp = StubKinodynamic()
    J, H, K = kinodynamic_values(nlp)
    call, remedy = not_replayable()[name]
    call(nlp, J, H, K)                                             # eagerly: runs, and warms whatever it launches
    assert nlp.engine.calls != []
    nlp.engine.calls.clear()
    tc.capturing = True
    with pytest.raises(RuntimeError, match="cannot be captured") as err:
        call(nlp, J, H, K)
    assert name in str(err.value) and remedy in str(err.value)
    assert nlp.engine.calls == []


POSE_NOT_REPLAYABLE = {
    "PoseNLP.__call__": lambda nlp: nlp(t(B, 81)),
    "PoseNLP.lagrangian_gradient": lambda nlp: nlp.lagrangian_gradient(t(B, 81), t(B), t(B, 4)),
    "PoseNLP.jacobian_vector_product": lambda nlp: nlp.jacobian_vector_product(t(B, 81), t(B, 81)),
    "PoseNLP.hessian_vector_product": lambda nlp: nlp.hessian_vector_product(t(B, 81), t(B), t(B, 4), t(B, 81)),
    "PoseNLP.kkt": lambda nlp: nlp.kkt(t(B, 81), 1.0, t(B, 4)),
    "set_params": lambda nlp: nlp.set_params(np.zeros((B, 202))),
}


@pytest.mark.parametrize("name", sorted(POSE_NOT_REPLAYABLE))
def test_what_is_not_replayable_on_the_pose_finder_is_refused_before_any_engine_call(monkeypatch, name):
    tc = Torch(monkeypatch)
    nlp = StubPose()
    POSE_NOT_REPLAYABLE[name](nlp)                                 # eagerly: runs
    assert nlp.engine.calls != []
    nlp.engine.calls.clear()
    tc.capturing = True
    with pytest.raises(RuntimeError, match="cannot be captured") as err:
        POSE_NOT_REPLAYABLE[name](nlp)
    assert name in str(err.value) and "outside the capture" in str(err.value)
    assert nlp.engine.calls == []


@pytest.mark.parametrize("make", [StubKinodynamic, StubPose])
def test_the_backward_passes_are_refused_while_capturing(monkeypatch, make):
    tc = Torch(monkeypatch)
    nlp = make()
    x = t(B, nlp.n).requires_grad_()
    f, g = nlp(x)                                                  # forward eagerly
    gx = nlp.lagrangian_gradient(x, t(B), t(B, nlp.m))             # recorded: its backward pass is the Hessian-vector product
    nlp.engine.calls.clear()
    tc.capturing = True
    with pytest.raises(RuntimeError, match="backward pass of nlp.x. cannot be captured"):
        (f.sum() + g.sum()).backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="double backward pass of nlp.x. cannot be captured"):
        gx.sum().backward(retain_graph=True)
    assert nlp.engine.calls == []
    tc.capturing = False
    (f.sum() + g.sum()).backward()
    assert nlp.engine.calls == ["eval_lagrangian_grad_device"]


# ---- 3. the cost of the guards --------------------------------------------------------------------------------------------------------------------
def test_a_warmed_replayable_method_asks_torch_nothing(monkeypatch):
    tc = Torch(monkeypatch)
    nlp = StubKinodynamic()
    J, H, K = kinodynamic_values(nlp)
    calls = kinodynamic_replayable()
    for name in sorted(calls):
        calls[name](nlp, J, H, K)
    assert tc.queries > 0                                          # (cold: every one asked)
    pre = K.block_preconditioner()
    pre.apply(t(B, nlp.n), t(B, nlp.m))
    K.solve(t(B, nlp.n), t(B, nlp.m), minv=pre, check_every=0)
    nlp.engine.calls.clear()
    tc.forbid_queries = True
    for name in sorted(calls):
        calls[name](nlp, J, H, K)
    pre.apply(t(B, nlp.n), t(B, nlp.m))
    K.solve(t(B, nlp.n), t(B, nlp.m), minv=pre, check_every=0)
    K.with_diagonals(None, None)
    assert len(nlp.engine.calls) >= len(calls)
    pose = StubPose()
    PK = pose_values(pose)
    tc.forbid_queries = False
    for name, call in sorted(pose_replayable().items()):
        call(pose, PK)
    tc.forbid_queries = True
    for name, call in sorted(pose_replayable().items()):
        call(pose, PK)


# ---- 4. the side stream -----------------------------------------------------------------------------------------------------------------------------
def test_the_side_stream_branch_is_never_taken_while_capturing(monkeypatch):
    """on the default stream (handle 0) a launch forks to the handle's side stream and joins: parallel branches in a graph"""
    tc = Torch(monkeypatch, handle=0)
    nlp = StubKinodynamic()
    autograd._warm_kinds(nlp).update(["hess_nnz", "kkt_times"])
    K = KKTValues(nlp, t(B, 13), t(B, 11))
    nlp.engine.calls.clear()
    tc.capturing = True
    with pytest.raises(RuntimeError, match="default stream"):      # (Stream.wait_stream would raise AssertionError: it was not reached)
        K.matvec(t(B, nlp.n), t(B, nlp.m))
    assert nlp.engine.calls == [] and getattr(nlp, "_side", None) is None



# ---- 5. the condition of the replay tests, where the emulation runs without a device ---------------------------------------------------------------
def _replay_refs(model, monkeypatch, name, horizon, lifted):
    import test_gpu_graph_replay as replay
    import test_gpu_kkt_minres as minres
    monkeypatch.setattr(minres, "dev", lambda a, dtype=None: None)       # (Inputs also makes device copies: not here)
    return replay, replay.refs_of(model, name, horizon, lifted, minres.Inputs)


def _cases():
    import test_gpu_graph_replay as replay
    return replay.CASES


@pytest.mark.parametrize("name,horizon,lifted", _cases())
def test_the_replay_tests_sets_a_and_b_expect_other_bytes_at_every_batch_position(model, monkeypatch, name, horizon, lifted):
    """tests/test_gpu_graph_replay.py asserts this before it replays anything; on the synthetic sets the emulation needs no device.  Set B
    is set A rolled by one along the batch axis.  Also what the solves' set is chosen for: trajectory 1 takes another number of
    iterations than trajectory 0, trajectory 2 (b = 0) has iteration 0 and status 0."""
    replay, r = _replay_refs(model, monkeypatch, name, horizon, lifted)
    Bs = replay.rolled(r.syn, 1)
    for what in replay.SYNTHETIC:
        a, b = r.product(what, r.syn), r.product(what, Bs)
        assert not replay.same_somewhere(a, b, range(len(a))), what
        for x, y in zip(a, b):
            assert np.array_equal(replay.raw(np.roll(x, 1, axis=0)), replay.raw(y)), what      # (the emulation is per trajectory)
    for kind in replay.SOLVES:
        a, b = r.solve(kind, r.syn), r.solve(kind, Bs)
        assert not replay.same_somewhere(a, b, (0, 1, 3)), kind
        its, status = a[2].tolist(), a[4].tolist()
        print(name, horizon, lifted, kind, "iterations", its, "status", status)
        assert status[2] == 0 and its[2] == 0 and its[0] > 0 and its[1] > 0, (kind, its, status)
        assert kind != "identity" or (status[:2] == [0, 0] and its[1] < its[0] < replay.MAXITER), (its, status)
        nan = {k: v.copy() for k, v in r.syn.items()}
        nan["bt"][0, 3] = np.nan
        assert r.solve(kind, nan)[4].tolist() == [2, status[1], status[2]], kind
