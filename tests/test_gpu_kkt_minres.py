"""GPU: preconditioned MINRES on the one-launch KKT operator, resident on the device (hipnlp_kkt_minres_device; the kernels
hipnlp_kkt_minres_apply_kernel / _first_kernel / _second_kernel; hippopt_amd.autograd.KKTValues.solve).  All six outputs equal the CPU
emulation (tests/kkt_minres_emu) bit for bit — for every check_every, with and without a preconditioner, in both jac orders, at every
batch position, with dx, dc or both omitted, at 100 and 300 knots, and on real value runs whatever their status; the true residual through KKTValues.matvec; freezing; the iteration limit;
guard words.  The synthetic inputs are those of tests/test_kkt_minres_hostemu.py (conditioned: no convergence is claimed on real iterates).
Batch 3: trajectory 0 as there, trajectory 1 with value runs of 0.02 standard_normal (converges earlier), trajectory 2 with b = 0."""
import numpy as np
import pytest

from kkt_check import bits
from test_lagrangian_grad_hostemu import MAKERS

pytestmark = pytest.mark.gpu
CASES = [("periodic", 2, False), ("cost_ends", 3, False), ("stairs", 3, False), ("single", 4, True)]      # (name, horizon, lifted)
B = 3
MAXITER = {False: 100, True: 300}
_EMU = {}


def dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def emu_of(model, name, horizon, lifted, vary_first=False):
    from kkt_minres_emu_lib import KktMinresEmu
    key = (name, horizon, lifted, vary_first)
    if key not in _EMU:
        _EMU[key] = KktMinresEmu(MAKERS[name](horizon, model), model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
    return _EMU[key]


class Inputs:
    """[B, ...] numpy inputs of a layout, and their device copies"""

    def __init__(self, emu, seed, same=False):
        rng = np.random.RandomState(seed)
        n, m = emu.n, emu.m
        sn = lambda *s: rng.standard_normal(s)  # noqa: E731
        self.hess, self.jac = sn(B, emu.nnz_h) * 0.05, sn(B, emu.nnz) * 0.05
        self.hess[1] *= 0.4
        self.jac[1] *= 0.4                                  # 0.02 standard_normal
        self.dx, self.dc = rng.uniform(1.0, 2.0, (B, n)), rng.uniform(1.0, 2.0, (B, m))
        self.bt, self.bb = sn(B, n), sn(B, m)
        self.bt[2], self.bb[2] = 0.0, 0.0
        self.mt, self.mb = rng.uniform(0.5, 2.0, (B, n)), rng.uniform(0.5, 2.0, (B, m))
        if same:
            for a in (self.hess, self.jac, self.dx, self.dc, self.bt, self.bb, self.mt, self.mb):
                a[1:] = a[0]
        self.d = {k: dev(getattr(self, k)) for k in ("hess", "jac", "dx", "dc", "bt", "bb", "mt", "mb")}

    def reference(self, emu, b, with_minv, rtol, maxiter, diagonals=(True, True)):
        return emu.solve(self.hess[b], self.jac[b], self.bt[b], self.bb[b], dx=self.dx[b] if diagonals[0] else None, dc=self.dc[b] if diagonals[1] else None, minv=(self.mt[b], self.mb[b]) if with_minv else None,
                         rtol=rtol, maxiter=maxiter)


def engine(model, name, horizon, lifted, vary_first=False):
    from hippopt_amd.hipnlp import HipNlp
    return HipNlp(MAKERS[name](horizon, model), model, batch=B, detect_simple_bounds=lifted, jac_varying_first=vary_first)


def solve(eng, inp, with_minv, rtol, maxiter, check_every, diagonals=(True, True)):
    """the six outputs of one solve into NaN / -99 destinations, as numpy"""
    import torch
    d = inp.d
    top, bottom = torch.full((B, eng.n), float("nan"), dtype=torch.float64, device="cuda"), torch.full((B, eng.m), float("nan"), dtype=torch.float64, device="cuda")
    res = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    its, status = torch.full((B,), -99, dtype=torch.int32, device="cuda"), torch.full((B,), -99, dtype=torch.int32, device="cuda")
    eng.kkt_minres_device(d["hess"].data_ptr(), d["jac"].data_ptr(), d["bt"].data_ptr(), d["bb"].data_ptr(), top.data_ptr(), bottom.data_ptr(), its.data_ptr(),
                          res.data_ptr(), status.data_ptr(), dx_ptr=d["dx"].data_ptr() if diagonals[0] else 0, dc_ptr=d["dc"].data_ptr() if diagonals[1] else 0,
                          minv_top_ptr=d["mt"].data_ptr() if with_minv else 0, minv_bottom_ptr=d["mb"].data_ptr() if with_minv else 0, rtol=rtol, max_iterations=maxiter, check_every=check_every, stream=stream())
    torch.cuda.synchronize()
    return top.cpu().numpy(), bottom.cpu().numpy(), its.cpu().numpy(), res.cpu().numpy(), status.cpu().numpy()


def assert_equals_emulation(got, ref, b, what):
    top, bottom, its, res, status = got
    print("%s b=%d: status %d / %d, iterations %d / %d, residual %.3e / %.3e (device / emulation)" % (what, b, status[b], ref.status, its[b], ref.iterations, res[b], ref.residual))
    assert (int(status[b]), int(its[b])) == (ref.status, ref.iterations), (what, b)
    assert bits(res[b:b + 1])[0] == bits([ref.residual])[0], (what, b, res[b], ref.residual)
    assert np.array_equal(bits(top[b]), bits(ref.top)), (what, b, "top", np.flatnonzero(bits(top[b]) != bits(ref.top))[:6])
    assert np.array_equal(bits(bottom[b]), bits(ref.bottom)), (what, b, "bottom", np.flatnonzero(bits(bottom[b]) != bits(ref.bottom))[:6])


# ---- 1. device == emulation, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_minv", [False, True])
@pytest.mark.parametrize("name,horizon,lifted,vary_first", [c + (False,) for c in CASES] + [("cost_ends", 3, False, True)])
def test_device_equals_the_emulation_bitwise(model, name, horizon, lifted, vary_first, with_minv):
    emu = emu_of(model, name, horizon, lifted, vary_first)
    eng = engine(model, name, horizon, lifted, vary_first)
    assert (emu.n, emu.m, emu.nnz, emu.nnz_h) == (eng.n, eng.m, eng.nnz, eng.hess_nnz())
    assert eng.kkt_minres_reserve() >= 6 * B * (eng.n + eng.m) * 8
    inp = Inputs(emu, 100 + horizon)
    maxiter = MAXITER[with_minv]
    refs = [inp.reference(emu, b, with_minv, 1e-8, maxiter) for b in range(B)]
    assert [r.status for r in refs] == [0, 0, 0] and (with_minv or refs[1].iterations < refs[0].iterations) and refs[2].iterations == 0
    for check_every in (0, 5):
        got = solve(eng, inp, with_minv, 1e-8, maxiter, check_every)
        for b in range(B):
            assert_equals_emulation(got, refs[b], b, "%s N=%d minv=%s check_every=%d" % (name, horizon, with_minv, check_every))


# ---- 1b. omitted diagonals, long horizons ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diagonals", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("name,horizon,lifted", [("cost_ends", 3, False), ("single", 4, True)])
def test_omitted_diagonals_equal_the_emulation_bitwise(model, name, horizon, lifted, diagonals):
    """dx, dc or both NULL: the apply launch reads the bottom of v for its partial although the operator does not.  These K are singular
    (tests/test_kkt_minres_hostemu.py): 25 iterations, no convergence asserted; also through KKTValues.with_diagonals(...).solve"""
    import torch
    from hippopt_amd.autograd import KKTValues, KinodynamicNLP
    emu, eng = emu_of(model, name, horizon, lifted), engine(model, name, horizon, lifted)
    inp = Inputs(emu, 600 + horizon)
    for with_minv in (False, True):
        got = solve(eng, inp, with_minv, 1e-8, 25, 0, diagonals)
        for b in range(B):
            ref = inp.reference(emu, b, with_minv, 1e-8, 25, diagonals)
            assert (ref.status, ref.iterations) == ((1, 25) if b < 2 else (0, 0))
            assert_equals_emulation(got, ref, b, "%s N=%d minv=%s diagonals=%s" % (name, horizon, with_minv, diagonals))
    d = inp.d
    nlp = KinodynamicNLP(MAKERS[name](horizon, model), model, batch=B, detect_simple_bounds=lifted)
    K = KKTValues(nlp, d["hess"], d["jac"], d["dx"], d["dc"]).with_diagonals(d["dx"] if diagonals[0] else None, d["dc"] if diagonals[1] else None)
    z = K.solve(d["bt"], d["bb"], maxiter=25, minv=(d["mt"], d["mb"]), check_every=5)
    torch.cuda.synchronize()
    for a, r in zip(z, got):
        assert np.array_equal(a.cpu().numpy().view(np.int64 if r.dtype == np.float64 else np.int32), r.view(np.int64 if r.dtype == np.float64 else np.int32))


@pytest.mark.parametrize("horizon,maxiter", [(100, 4), (300, 3)])
def test_long_horizons_sum_their_partials_in_the_emulations_order(model, horizon, maxiter):
    """more than 64 and more than 256 knots: the partials of a trajectory come to the first wave in four registers per lane and in more
    than one round; the bits stay those of the plain loop of the emulation"""
    emu, eng = emu_of(model, "periodic", horizon, False), engine(model, "periodic", horizon, False)
    inp = Inputs(emu, 700 + horizon)
    got = solve(eng, inp, True, 1e-8, maxiter, 0)
    for b in range(B):
        ref = inp.reference(emu, b, True, 1e-8, maxiter)
        assert (ref.status, ref.iterations) == ((1, maxiter) if b < 2 else (0, 0))
        assert_equals_emulation(got, ref, b, "periodic N=%d maxiter=%d" % (horizon, maxiter))


# ---- 2. batch positions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,horizon,lifted", CASES)
def test_batch_positions_give_the_same_bits(model, name, horizon, lifted):
    emu, eng = emu_of(model, name, horizon, lifted), engine(model, name, horizon, lifted)
    inp = Inputs(emu, 200 + horizon, same=True)
    top, bottom, its, res, status = solve(eng, inp, True, 1e-8, 300, 16)
    assert status[0] == 0 and its[0] > 0
    for b in (1, 2):
        assert np.array_equal(bits(top[b]), bits(top[0])) and np.array_equal(bits(bottom[b]), bits(bottom[0]))
        assert (its[b], status[b]) == (its[0], status[0]) and bits(res)[b] == bits(res)[0]


# ---- 3. the true residual, through the torch entry points ------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_minv", [False, True])
@pytest.mark.parametrize("name,horizon,lifted", CASES)
def test_true_residual_through_the_operator(model, name, horizon, lifted, with_minv):
    import torch
    from hippopt_amd.autograd import KKTSolution, KKTValues, KinodynamicNLP
    emu = emu_of(model, name, horizon, lifted)
    inp = Inputs(emu, 300 + horizon)
    d = inp.d
    nlp = KinodynamicNLP(MAKERS[name](horizon, model), model, batch=B, detect_simple_bounds=lifted)
    K = KKTValues(nlp, d["hess"], d["jac"], d["dx"], d["dc"])
    minv = (d["mt"], d["mb"]) if with_minv else None
    for rtol in (1e-8, 1e-12):
        z = K.solve(d["bt"], d["bb"], rtol=rtol, maxiter=MAXITER[with_minv], minv=minv)
        assert isinstance(z, KKTSolution) and z.iterations.dtype == torch.int32 and z.status.dtype == torch.int32 and not z.top.requires_grad
        kt, kb = K.matvec(z.top, z.bottom)
        r, b = torch.cat([d["bt"] - kt, d["bb"] - kb], dim=1), torch.cat([d["bt"], d["bb"]], dim=1)
        mi = torch.cat(minv, dim=1) if with_minv else torch.ones_like(r)
        true = (torch.sqrt((r * mi * r).sum(1)) / torch.sqrt((b * mi * b).sum(1)).clamp_min(1e-300)).cpu().numpy()
        est, status, its = z.residual.cpu().numpy(), z.status.cpu().numpy(), z.iterations.cpu().numpy()
        print("%s N=%d minv=%s rtol=%g: iterations %s, residual %s, true %s" % (name, horizon, with_minv, rtol, its, est, true))
        assert np.all(status == 0) and its[2] == 0 and np.all(its[:2] > 0)
        assert np.all(true <= 2.0 * rtol) and np.all(np.abs(est - true) <= rtol)


# ---- 4. / 5. freezing and the iteration limit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,horizon,lifted", CASES)
def test_frozen_trajectories_and_the_iteration_limit(model, name, horizon, lifted):
    emu, eng = emu_of(model, name, horizon, lifted), engine(model, name, horizon, lifted)
    inp = Inputs(emu, 400 + horizon)
    a, b = solve(eng, inp, False, 1e-8, 100, 0), solve(eng, inp, False, 1e-8, 140, 0)
    assert np.all(a[4] == 0) and np.all(a[2] < 100)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
    top, bottom, its, res, status = solve(eng, inp, False, 1e-8, 5, 0)
    assert list(status) == [1, 1, 0] and list(its) == [5, 5, 0] and np.all(res[:2] > 1e-8) and res[2] == 0.0
    for bb in range(B):
        assert_equals_emulation((top, bottom, its, res, status), inp.reference(emu, bb, False, 1e-8, 5), bb, "%s N=%d maxiter=5" % (name, horizon))


# ---- 6. destinations ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,horizon,lifted", CASES)
def test_guard_words_stay(model, name, horizon, lifted):
    import torch
    emu, eng = emu_of(model, name, horizon, lifted), engine(model, name, horizon, lifted)
    inp = Inputs(emu, 500 + horizon)
    d, G = inp.d, 256
    big = {k: torch.full((words + 2 * G,), float("nan"), dtype=torch.float64, device="cuda") for k, words in (("top", B * eng.n), ("bottom", B * eng.m), ("res", B))}
    ints = {k: torch.full((B + 2 * G,), -77, dtype=torch.int32, device="cuda") for k in ("its", "status")}
    P = lambda t, size: t.data_ptr() + size * G  # noqa: E731
    eng.kkt_minres_device(d["hess"].data_ptr(), d["jac"].data_ptr(), d["bt"].data_ptr(), d["bb"].data_ptr(), P(big["top"], 8), P(big["bottom"], 8), P(ints["its"], 4),
                          P(big["res"], 8), P(ints["status"], 4), dx_ptr=d["dx"].data_ptr(), dc_ptr=d["dc"].data_ptr(), rtol=1e-8, max_iterations=100, check_every=16,
                          stream=stream())
    torch.cuda.synchronize()
    for k, t in big.items():
        h = t.cpu().numpy()
        assert np.all(np.isnan(h[:G])) and np.all(np.isnan(h[-G:])), k
        assert np.all(np.isfinite(h[G:-G])), k
    for k, t in ints.items():
        h = t.cpu().numpy()
        assert np.all(h[:G] == -77) and np.all(h[-G:] == -77) and np.all(h[G:-G] >= 0), k
    ref = inp.reference(emu, 0, False, 1e-8, 100)
    assert np.array_equal(bits(big["top"].cpu().numpy()[G:G + eng.n]), bits(ref.top))


# ---- 7. real value runs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["periodic", "stairs"])
def test_real_value_runs_equal_the_emulation_whatever_the_status(model, name):
    """the KKT system of a synthetic workload's iterate, N = 4: indefinite and badly scaled, 20 iterations without a preconditioner.
    No convergence is asserted — only that device and emulation agree on every bit of every output."""
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    from hippopt_amd.synthetic import make_workload, place_on_step_flanks
    st = MAKERS[name](4, model)
    x, p = make_workload(st, model, batch=B, seed=8900)
    if name == "stairs":
        place_on_step_flanks(x[:1], st, seed=3)
    nlp = KinodynamicNLP(st, model, batch=B)
    nlp.set_params(p)
    emu = emu_of(model, name, 4, False)
    rng = np.random.RandomState(11)
    lam, dx, dc = rng.standard_normal((B, nlp.m)), rng.uniform(1.0, 2.0, (B, nlp.n)), rng.uniform(1.0, 2.0, (B, nlp.m))
    bt, bb = rng.standard_normal((B, nlp.n)), rng.standard_normal((B, nlp.m))
    K = nlp.kkt(dev(x), 0.8, dev(lam), dev(dx), dev(dc))
    z = K.solve(dev(bt), dev(bb), rtol=1e-8, maxiter=20, check_every=0)
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in z)
    hess, jac = K.hess.cpu().numpy(), K.jac.cpu().numpy()
    print("%s: |hess| up to %.3e, |jac| up to %.3e" % (name, np.abs(hess).max(), np.abs(jac).max()))
    for b in range(B):
        ref = emu.solve(hess[b], jac[b], bt[b], bb[b], dx=dx[b], dc=dc[b], rtol=1e-8, maxiter=20)
        assert_equals_emulation(got, ref, b, "%s N=4 real value runs" % name)
