"""GPU: the block preconditioner of the KKT solve (hipnlp_kkt_block_factor_device, hipnlp_kkt_block_apply_device,
hipnlp_kkt_minres_block_device; hippopt_amd.autograd.KKTValues.block_preconditioner).  The stored factor, pivot words, e, o, inertia and
status, the apply and the whole solve equal the CPU emulation (tests/kkt_block_emu) bit for bit — on synthetic value runs of every maker at
N = 2, 3, 4 (N = 2: first and last knots only; N = 4: all four pair variants), in both jac orders, lifted, and on the device's own real
value runs at N = 4; batch 3 with inputs that differ per trajectory (a wrong batch stride of the 143 KB records shows).  A NaN in one
knot's Hessian values (data through a normal launch) gives status 2 for that knot only; every output word is written; a second build on
the same handle equals a fresh handle's; one case at 100 knots x 2."""
import numpy as np
import pytest

from kkt_check import bits
from test_lagrangian_grad_hostemu import MAKERS

pytestmark = pytest.mark.gpu
SMALL = [(name, horizon, False, False) for name in MAKERS for horizon in (2, 3, 4)]
CASES = SMALL + [("periodic", 3, False, True), ("cost_ends", 2, False, True), ("single", 4, True, False)]      # (name, horizon, lifted, vary_first)
SOLVES = [("periodic", 2, False, False), ("stairs", 4, False, False), ("cost_ends", 3, False, True), ("single", 4, True, False)]
B = 3
NXK = 189
FLOOR = 1e-10
_EMU = {}


def dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def emu_of(model, name, horizon, lifted, vary_first=False):
    from kkt_block_emu_lib import KktBlockEmu
    key = (name, horizon, lifted, vary_first)
    if key not in _EMU:
        _EMU[key] = KktBlockEmu(MAKERS[name](horizon, model), model, detect_simple_bounds=lifted, jac_varying_first=vary_first)
    return _EMU[key]


def nlp_of(model, name, horizon, lifted, vary_first=False, batch=B):
    from hippopt_amd.autograd import KinodynamicNLP
    from hippopt_amd.hipnlp import HipNlp
    nlp = KinodynamicNLP(MAKERS[name](horizon, model), model, batch=batch, detect_simple_bounds=lifted)
    if vary_first:                                                              # (the other jac order is the engine's option: the same n, m and patterns' sizes)
        nlp.engine = HipNlp(MAKERS[name](horizon, model), model, batch=batch, detect_simple_bounds=lifted, jac_varying_first=True)
    return nlp


def synthetic(emu, seed, batch=B):
    """the conditioned synthetic runs of tests/test_kkt_minres_hostemu.py, different per trajectory; trajectory 1 with a Hessian 40 times
    larger: |H| up to about 8 against dx in [1, 2], so its blocks are indefinite and 2x2 pivots occur"""
    rng = np.random.RandomState(seed)
    d = dict(hess=0.05 * rng.standard_normal((batch, emu.nnz_h)), jac=0.05 * rng.standard_normal((batch, emu.nnz)), dx=rng.uniform(1.0, 2.0, (batch, emu.n)),
             dc=rng.uniform(1.0, 2.0, (batch, emu.m)), bt=rng.standard_normal((batch, emu.n)), bb=rng.standard_normal((batch, emu.m)))
    d["hess"][1] *= 40.0
    return d


def assert_block_equals(M, emu, d, b, what, dx=True):
    """the six stored arrays of trajectory b against the emulation; returns the emulation's Block and Diagonal"""
    ref = emu.block_factor(d["hess"][b], d["dx"][b] if dx else None, FLOOR)
    diag = emu.diagonal_preconditioner(d["hess"][b], d["jac"][b], d["dx"][b] if dx else None, d["dc"][b], FLOOR)
    assert ref.det_not_negative == 0 and ref.not_positive_definite == 0, what
    assert np.array_equal(M.status[b].cpu().numpy(), ref.status), (what, "status")
    assert np.array_equal(M.inertia[b].cpu().numpy(), ref.inertia), (what, "inertia", M.inertia[b].cpu().numpy().tolist(), ref.inertia.tolist())
    assert np.array_equal(M.pivots[b].cpu().numpy(), ref.words), (what, "pivot words")
    for name, got, want in (("factor", M.factor[b], ref.factor), ("e", M.e[b], ref.e), ("o", M.o[b], ref.o), ("top diagonal", M.top_diagonal[b], diag.top),
                            ("bottom", M.bottom[b], diag.bottom)):
        got = got.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (what, name, np.argwhere(bits(got) != bits(want))[:4].tolist())
    return ref, diag


# ---- 1. device == emulation, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,horizon,lifted,vary_first", CASES)
def test_factor_and_apply_equal_the_emulation_bitwise(model, name, horizon, lifted, vary_first):
    import torch
    from hippopt_amd.autograd import KKTValues
    emu, nlp = emu_of(model, name, horizon, lifted, vary_first), nlp_of(model, name, horizon, lifted, vary_first)
    assert (emu.n, emu.m, emu.nnz, emu.nnz_h) == (nlp.n, nlp.m, nlp.engine.nnz, nlp.engine.hess_nnz())
    d = synthetic(emu, 1600 + horizon)
    K = KKTValues(nlp, dev(d["hess"]), dev(d["jac"]), dev(d["dx"]), dev(d["dc"]))
    M = K.block_preconditioner(FLOOR)
    assert M.factor.shape == (B, horizon, NXK * (NXK + 1) // 2) and M.pivots.shape == M.e.shape == M.o.shape == (B, horizon, NXK)
    assert M.inertia.shape == (B, horizon, 3) and M.status.shape == (B, horizon)
    assert nlp.engine.kkt_block_bytes() == (M.factor.numel() * 8, M.pivots.numel() * 4, M.e.numel() * 8, M.o.numel() * 8)
    zt, zb = M.apply(dev(d["bt"]), dev(d["bb"]))
    torch.cuda.synchronize()
    assert int(M.inertia[1, :, 1].sum()) > 0                                    # trajectory 1 has negative eigenvalues
    for b in range(B):
        what = "%s N=%d lifted=%s vary_first=%s b=%d" % (name, horizon, lifted, vary_first, b)
        ref, diag = assert_block_equals(M, emu, d, b, what)
        assert np.all(ref.status == 0) and np.all(ref.inertia.sum(axis=1) == NXK)
        app = emu.block_apply(ref, (diag.top, diag.bottom), d["bt"][b], d["bb"][b])
        assert np.all(app.top_writes == 1) and np.all(app.bottom_writes == 1)
        assert np.array_equal(bits(zt[b].cpu().numpy()), bits(app.top)), (what, "apply top", np.flatnonzero(bits(zt[b].cpu().numpy()) != bits(app.top))[:6])
        assert np.array_equal(bits(zb[b].cpu().numpy()), bits(app.bottom)), (what, "apply bottom")
    # without dx: H_k alone
    M0 = K.with_diagonals(None, dev(d["dc"])).block_preconditioner(FLOOR)
    torch.cuda.synchronize()
    assert_block_equals(M0, emu, d, 1, "%s N=%d without dx" % (name, horizon), dx=False)


def solve_equals(K, M, emu, refs, d, maxiter, what):
    import torch
    for check_every in (0, 7):
        z = K.solve(dev(d["bt"]), dev(d["bb"]), rtol=1e-8, maxiter=maxiter, minv=M, check_every=check_every)
        torch.cuda.synchronize()
        top, bottom, its, res, status = (a.cpu().numpy() for a in z)
        for b, ref in enumerate(refs):
            w = "%s check_every=%d b=%d" % (what, check_every, b)
            print("%s: status %d / %d, iterations %d / %d, residual %.3e / %.3e (device / emulation)" % (w, status[b], ref.status, its[b], ref.iterations, res[b], ref.residual))
            assert (int(status[b]), int(its[b])) == (ref.status, ref.iterations), w
            assert bits(res[b:b + 1])[0] == bits([ref.residual])[0], w
            assert np.array_equal(bits(top[b]), bits(ref.top)) and np.array_equal(bits(bottom[b]), bits(ref.bottom)), w


@pytest.mark.parametrize("name,horizon,lifted,vary_first", SOLVES)
def test_solve_with_the_block_preconditioner_equals_the_emulation(model, name, horizon, lifted, vary_first):
    from hippopt_amd.autograd import KKTValues
    emu, nlp = emu_of(model, name, horizon, lifted, vary_first), nlp_of(model, name, horizon, lifted, vary_first)
    d = synthetic(emu, 1700 + horizon)
    K = KKTValues(nlp, dev(d["hess"]), dev(d["jac"]), dev(d["dx"]), dev(d["dc"]))
    M = K.block_preconditioner(FLOOR)
    refs = []
    for b in range(B):
        ref, diag = assert_block_equals(M, emu, d, b, "%s N=%d b=%d" % (name, horizon, b))
        refs.append(emu.block_solve(d["hess"][b], d["jac"][b], d["bt"][b], d["bb"][b], ref, (diag.top, diag.bottom), dx=d["dx"][b], dc=d["dc"][b], rtol=1e-8, maxiter=60))
    assert refs[0].status == 0 and 0 < refs[0].iterations < 60                  # the conditioned trajectory converges
    solve_equals(K, M, emu, refs, d, 60, "%s N=%d" % (name, horizon))


@pytest.mark.parametrize("name", ["periodic", "stairs"])
def test_real_value_runs_equal_the_emulation(model, name):
    """the KKT system of a synthetic workload's iterate at N = 4 (tests/test_gpu_kkt_precond.py's), on the device's own value runs: the
    stored arrays, the apply, and 25 iterations of the solve, whatever the status"""
    import torch
    from hippopt_amd.synthetic import make_workload, place_on_step_flanks
    st = MAKERS[name](4, model)
    x, p = make_workload(st, model, batch=B, seed=8900)
    if name == "stairs":
        place_on_step_flanks(x[:1], st, seed=3)
    nlp = nlp_of(model, name, 4, False)
    nlp.set_params(p)
    emu = emu_of(model, name, 4, False)
    rng = np.random.RandomState(11)
    lam, dx, dc = rng.standard_normal((B, nlp.m)), rng.uniform(1.0, 2.0, (B, nlp.n)), rng.uniform(1.0, 2.0, (B, nlp.m))
    d = dict(dx=dx, dc=dc, bt=rng.standard_normal((B, nlp.n)), bb=rng.standard_normal((B, nlp.m)))
    K = nlp.kkt(dev(x), 0.8, dev(lam), dev(dx), dev(dc))
    M = K.block_preconditioner(FLOOR)
    zt, zb = M.apply(dev(d["bt"]), dev(d["bb"]))
    torch.cuda.synchronize()
    d["hess"], d["jac"] = K.hess.cpu().numpy(), K.jac.cpu().numpy()
    print("%s: |hess| up to %.3e, inertia %s" % (name, np.abs(d["hess"]).max(), M.inertia.cpu().numpy().tolist()))
    refs = []
    for b in range(B):
        ref, diag = assert_block_equals(M, emu, d, b, "%s real b=%d" % (name, b))
        app = emu.block_apply(ref, (diag.top, diag.bottom), d["bt"][b], d["bb"][b])
        assert np.array_equal(bits(zt[b].cpu().numpy()), bits(app.top)) and np.array_equal(bits(zb[b].cpu().numpy()), bits(app.bottom)), (name, b)
        refs.append(emu.block_solve(d["hess"][b], d["jac"][b], d["bt"][b], d["bb"][b], ref, (diag.top, diag.bottom), dx=dx[b], dc=dc[b], rtol=1e-8, maxiter=25))
    solve_equals(K, M, emu, refs, d, 25, "%s real" % name)


# ---- 2. NaN data ------------------------------------------------------------------------------------------------------------------------------
def test_a_nan_in_one_knot_gives_status_2_for_that_knot_only(model):
    """NaN data through a normal launch: trajectory 1, knot 2 of four"""
    import torch
    from hippopt_amd.autograd import KKTValues
    name, horizon = "stairs", 4
    emu, nlp = emu_of(model, name, horizon, False), nlp_of(model, name, horizon, False)
    d = synthetic(emu, 1800)
    nnz_knot = emu.block_pattern()[1].size
    d["hess"][1, 2 * nnz_knot + 5] = np.nan
    K = KKTValues(nlp, dev(d["hess"]), dev(d["jac"]), dev(d["dx"]), dev(d["dc"]))
    M = K.block_preconditioner(FLOOR)
    zt, zb = M.apply(dev(d["bt"]), dev(d["bb"]))
    z = K.solve(dev(d["bt"]), dev(d["bb"]), rtol=1e-8, maxiter=60, minv=M, check_every=7)
    torch.cuda.synchronize()
    want = np.zeros((B, horizon), np.int32)
    want[1, 2] = 2
    assert np.array_equal(M.status.cpu().numpy(), want)
    assert M.inertia[1, 2].cpu().numpy().tolist() == [0, 0, 0]
    for b in range(B):
        assert_block_equals(M, emu, d, b, "NaN case b=%d" % b)
    nan = torch.isnan(zt).cpu().numpy()
    expect = np.zeros((B, nlp.n), bool)
    expect[1, 2 * NXK:3 * NXK] = True
    assert np.array_equal(nan, expect) and not torch.isnan(zb).any()
    assert z.status.cpu().numpy().tolist() == [0, 2, 0] and int(z.iterations[1]) == 0


# ---- 3. writes and reuse ------------------------------------------------------------------------------------------------------------------------
def test_every_output_word_is_written_and_guard_words_stay(model):
    import torch
    name, horizon = "cost_ends", 3
    emu, nlp = emu_of(model, name, horizon, False), nlp_of(model, name, horizon, False)
    eng = nlp.engine
    d = synthetic(emu, 1900)
    G, SENT, ISENT = 64, -7.25e300, -77
    nb = eng.kkt_block_bytes()
    f = torch.full((nb[0] // 8 + 2 * G,), SENT, dtype=torch.float64, device="cuda")
    p = torch.full((nb[1] // 4 + 2 * G,), ISENT, dtype=torch.int32, device="cuda")
    e, o = (torch.full((nb[2] // 8 + 2 * G,), SENT, dtype=torch.float64, device="cuda") for _ in range(2))
    inertia = torch.full((B * horizon * 3 + 2 * G,), ISENT, dtype=torch.int32, device="cuda")
    status = torch.full((B * horizon + 2 * G,), ISENT, dtype=torch.int32, device="cuda")
    hess, dx = dev(d["hess"]), dev(d["dx"])
    eng.kkt_block_factor_device(hess.data_ptr(), f.data_ptr() + 8 * G, p.data_ptr() + 4 * G, e.data_ptr() + 8 * G, o.data_ptr() + 8 * G, inertia.data_ptr() + 4 * G,
                                status.data_ptr() + 4 * G, dx_ptr=dx.data_ptr(), floor=FLOOR, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for t, sent in ((f, SENT), (p, ISENT), (e, SENT), (o, SENT), (inertia, ISENT), (status, ISENT)):
        a = t.cpu().numpy()
        assert np.all(a[:G] == sent) and np.all(a[-G:] == sent)                  # guard words
        assert not np.any(a[G:-G] == sent)                                       # every word written
    ref = emu.block_factor(d["hess"][2], d["dx"][2], FLOOR)
    got = f.cpu().numpy()[G:-G].reshape(B, horizon, -1)[2]
    assert np.array_equal(bits(got), bits(ref.factor))


def test_a_second_build_on_the_same_handle_equals_a_fresh_handle(model):
    import torch
    from hippopt_amd.autograd import KKTValues
    name, horizon = "periodic", 4
    emu = emu_of(model, name, horizon, False)
    d, other = synthetic(emu, 2000), synthetic(emu, 2001)
    nlp = nlp_of(model, name, horizon, False)
    K = KKTValues(nlp, dev(d["hess"]), dev(d["jac"]), dev(d["dx"]), dev(d["dc"]))
    first = K.block_preconditioner(FLOOR)
    second = K.with_diagonals(dev(other["dx"]), dev(other["dc"])).block_preconditioner(FLOOR)
    fresh = KKTValues(nlp_of(model, name, horizon, False), dev(d["hess"]), dev(d["jac"]), dev(other["dx"]), dev(other["dc"])).block_preconditioner(FLOOR)
    torch.cuda.synchronize()
    assert not torch.equal(first.factor, second.factor)
    for a in ("factor", "pivots", "e", "o", "inertia", "status", "top_diagonal", "bottom"):
        got, want = getattr(second, a).cpu().numpy(), getattr(fresh, a).cpu().numpy()
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), a


# ---- 4. a full-occupancy shape ------------------------------------------------------------------------------------------------------------------
def test_one_hundred_knots_equal_the_emulation(model):
    """100 knots x 2 trajectories: the factor launch and one apply against the emulation (no solve)"""
    import torch
    from hippopt_amd.autograd import KKTValues
    name, horizon, batch = "periodic", 100, 2
    emu, nlp = emu_of(model, name, horizon, False), nlp_of(model, name, horizon, False, batch=batch)
    d = synthetic(emu, 2100, batch=batch)
    K = KKTValues(nlp, dev(d["hess"]), dev(d["jac"]), dev(d["dx"]), dev(d["dc"]))
    M = K.block_preconditioner(FLOOR)
    zt, zb = M.apply(dev(d["bt"]), dev(d["bb"]))
    torch.cuda.synchronize()
    for b in range(batch):
        ref, diag = assert_block_equals(M, emu, d, b, "N=100 b=%d" % b)
        app = emu.block_apply(ref, (diag.top, diag.bottom), d["bt"][b], d["bb"][b])
        assert np.array_equal(bits(zt[b].cpu().numpy()), bits(app.top)) and np.array_equal(bits(zb[b].cpu().numpy()), bits(app.bottom))
