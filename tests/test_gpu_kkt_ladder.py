"""GPU: the per-knot inertia-correcting ladder of the block factorisation (hipnlp_kkt_block_ladder_device;
hippopt_amd.autograd.KKTValues.convexify).  The stored factor, pivot words, e, o, inertia, status, delta and tries equal the CPU emulation
(tests/kkt_ladder_emu) bit for bit on the device's own real value runs at N = 4 (stairs, periodic) and N = 2 (first and last knot only),
batch 3 with a dx that differs per trajectory by factors of 100 — so the knots of one launch leave the ladder at different tries — with a
NaN knot in trajectory 1, and in three ladder configurations: convexify's defaults, one that exhausts some knots and not others, and one
try of a tiny delta that exhausts all.  max_tries = 0 equals hipnlp_kkt_block_factor_device's six arrays bitwise.  Through torch:
K.convexify() is quasi-definite on the real runs, its .values carry dx + delta per knot with the globals untouched, its apply and a short
solve on .values equal the emulation's bits.  A multi-device handle and a shard handle get HIPNLP_E_UNSUPPORTED from both entry points."""
import numpy as np
import pytest

from kkt_check import bits
from test_lagrangian_grad_hostemu import MAKERS

pytestmark = pytest.mark.gpu
B = 3
NXK = 189
FLOOR = 1e-10
E_UNSUPPORTED = -6
DX_SCALE = (1.0, 100.0, 1e4)                                                     # per trajectory
CONFIGS = [(1e-4, 8.0, 16), (1e-3, 2.0, 16), (1e-300, 8.0, 1)]                   # (delta_init, kappa, max_tries)
RUNS = [("stairs", 4), ("periodic", 4), ("stairs", 2), ("periodic", 2)]
_EMU, _REAL = {}, {}


def dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def emu_of(model, name, horizon):
    from kkt_ladder_emu_lib import KktLadderEmu
    if (name, horizon) not in _EMU:
        _EMU[name, horizon] = KktLadderEmu(MAKERS[name](horizon, model), model)
    return _EMU[name, horizon]


def real(model, name, horizon):
    """(nlp, K, inputs as numpy) of the KKT system of a synthetic workload's iterate (tests/test_gpu_kkt_block.py's), on the device's own
    value runs, computed once; dx of trajectory b scaled by DX_SCALE[b]"""
    import torch
    from hippopt_amd.autograd import KinodynamicNLP
    from hippopt_amd.synthetic import make_workload, place_on_step_flanks
    if (name, horizon) not in _REAL:
        st = MAKERS[name](horizon, model)
        x, p = make_workload(st, model, batch=B, seed=8900)
        if name == "stairs":
            place_on_step_flanks(x[:1], st, seed=3)
        nlp = KinodynamicNLP(st, model, batch=B)
        nlp.set_params(p)
        rng = np.random.RandomState(11)
        lam, dx, dc = rng.standard_normal((B, nlp.m)), rng.uniform(1.0, 2.0, (B, nlp.n)), rng.uniform(1.0, 2.0, (B, nlp.m))
        dx *= np.asarray(DX_SCALE)[:, None]
        d = dict(dx=dx, dc=dc, bt=rng.standard_normal((B, nlp.n)), bb=rng.standard_normal((B, nlp.m)))
        K = nlp.kkt(dev(x), 0.8, dev(lam), dev(dx), dev(dc))
        torch.cuda.synchronize()
        d["hess"], d["jac"] = K.hess.cpu().numpy(), K.jac.cpu().numpy()
        _REAL[name, horizon] = (nlp, K, d)
    return _REAL[name, horizon]


class Arrays:
    """the eight outputs of one ladder launch, pre-filled with sentinels"""

    def __init__(self, nlp, horizon):
        import torch
        nb = nlp.engine.kkt_block_bytes()
        full = lambda shape, v, t: torch.full(shape, v, dtype=t, device="cuda")  # noqa: E731
        self.factor = full((B, horizon, nb[0] // (8 * B * horizon)), -7.25e300, torch.float64)
        self.pivots = full((B, horizon, NXK), -77, torch.int32)
        self.e, self.o = full((B, horizon, NXK), -7.25e300, torch.float64), full((B, horizon, NXK), -7.25e300, torch.float64)
        self.inertia, self.status = full((B, horizon, 3), -77, torch.int32), full((B, horizon), -77, torch.int32)
        self.delta, self.tries = full((B, horizon), -7.25e300, torch.float64), full((B, horizon), -77, torch.int32)

    def six(self):
        return [self.factor, self.pivots, self.e, self.o, self.inertia, self.status]


def launch_ladder(nlp, horizon, hess, dx, delta_init, kappa, max_tries):
    import torch
    out = Arrays(nlp, horizon)
    nlp.engine.kkt_block_ladder_device(hess.data_ptr(), *(t.data_ptr() for t in out.six()), out.delta.data_ptr(), out.tries.data_ptr(), dx_ptr=dx.data_ptr() if dx is not None else 0,
                                       floor=FLOOR, delta_init=delta_init, kappa=kappa, max_tries=max_tries, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def assert_ladder_equals(out, ref, b, what):
    """trajectory b of a launch's eight arrays (or of a KKTBlockPreconditioner) against the emulation's Ladder"""
    for name, got, want in (("status", out.status, ref.status), ("tries", out.tries, ref.tries), ("inertia", out.inertia, ref.inertia), ("pivot words", out.pivots, ref.words)):
        assert np.array_equal(got[b].cpu().numpy(), want), (what, name, got[b].cpu().numpy().tolist()[:8], want.tolist()[:8])
    for name, got, want in (("delta", out.delta, ref.delta), ("factor", out.factor, ref.factor), ("e", out.e, ref.e), ("o", out.o, ref.o)):
        got = got[b].cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (what, name, np.argwhere(bits(got) != bits(want))[:4].tolist())


# ---- 1. device == emulation, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,horizon", RUNS)
def test_the_ladder_equals_the_emulation_bitwise(model, name, horizon):
    emu = emu_of(model, name, horizon)
    nlp, K, d = real(model, name, horizon)
    assert (emu.n, emu.m, emu.nnz, emu.nnz_h) == (nlp.n, nlp.m, nlp.engine.nnz, nlp.engine.hess_nnz())
    nnz_knot = emu.block_pattern()[1].size
    hess = d["hess"].copy()
    nan_knot = horizon - 2
    hess[1, nan_knot * nnz_knot + 5] = np.nan                                    # NaN data through a normal launch: trajectory 1
    seen = set()
    for delta_init, kappa, max_tries in CONFIGS:
        out = launch_ladder(nlp, horizon, dev(hess), K.dx, delta_init, kappa, max_tries)
        status, tries = out.status.cpu().numpy(), out.tries.cpu().numpy()
        print("%s N=%d delta_init %g kappa %g max_tries %d: status %s tries %s" % (name, horizon, delta_init, kappa, max_tries, status.tolist(), tries.tolist()))
        for b in range(B):
            ref = emu.block_ladder(hess[b], d["dx"][b], FLOOR, delta_init, kappa, max_tries)
            assert ref.det_not_negative == 0 and ref.not_positive_definite == 0
            assert_ladder_equals(out, ref, b, "%s N=%d b=%d %r" % (name, horizon, b, (delta_init, kappa, max_tries)))
        assert status[1, nan_knot] == 2 and tries[1, nan_knot] == 0 and (status[1] == 2).sum() == 1
        assert out.inertia[1, nan_knot].cpu().numpy().tolist() == [0, 0, 0] and bool(out.factor[1, nan_knot].isnan().all())
        seen |= set(status.ravel().tolist())
        if max_tries == 16 and delta_init == 1e-4:
            ok = status == 0
            assert np.all(out.inertia.cpu().numpy()[ok] == [NXK, 0, 0]) and ok.sum() == B * horizon - 1
            assert len(set(tries[0].tolist()) | set(tries[2].tolist())) > 1      # knots of one launch leave at different tries
        if max_tries == 1:
            assert np.all(status[0] == 3) and np.all(tries[0] == 1)               # trajectory 0 (dx in U[1, 2]): every knot exhausted
    assert seen == {0, 2, 3}


def test_without_dx_and_with_no_tries_the_ladder_is_the_factor_launch(model):
    """max_tries = 0 against hipnlp_kkt_block_factor_device on the same handle: the six arrays bitwise, delta 0, tries 0"""
    import torch
    name, horizon = "stairs", 4
    nlp, K, d = real(model, name, horizon)
    for dx in (K.dx, None):
        out = launch_ladder(nlp, horizon, K.hess, dx, 0.0, 0.0, 0)               # (delta_init and kappa are not read)
        want = Arrays(nlp, horizon)
        nlp.engine.kkt_block_factor_device(K.hess.data_ptr(), *(t.data_ptr() for t in want.six()), dx_ptr=dx.data_ptr() if dx is not None else 0, floor=FLOOR,
                                           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for got, ref in zip(out.six(), want.six()):
            assert np.array_equal(got.cpu().numpy().view(np.uint8), ref.cpu().numpy().view(np.uint8))
        assert int(out.inertia[:, :, 1].sum()) > 0 and bool((out.status == 0).all())  # status 0 whatever the inertia
        assert bool((out.tries == 0).all()) and np.all(bits(out.delta.cpu().numpy()) == 0)
    ref = emu_of(model, name, horizon).block_ladder(d["hess"][2], None, FLOOR, 1e-4, 8.0, 16)
    assert_ladder_equals(launch_ladder(nlp, horizon, K.hess, None, 1e-4, 8.0, 16), ref, 2, "without dx")


# ---- 2. through torch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stairs", "periodic"])
def test_convexify_through_torch_equals_the_emulation(model, name):
    import torch
    horizon = 4
    emu = emu_of(model, name, horizon)
    nlp, K, d = real(model, name, horizon)
    pre = K.convexify(floor=FLOOR)                                               # the defaults: 1e-4, 8, 16
    zt, zb = pre.apply(dev(d["bt"]), dev(d["bb"]))
    torch.cuda.synchronize()
    assert pre.quasi_definite.dtype == torch.bool and pre.quasi_definite.cpu().numpy().tolist() == [True] * B
    assert pre.delta.shape == pre.tries.shape == pre.status.shape == (B, horizon) and pre.tries.dtype == torch.int32
    assert pre.values is not K and pre.values.hess is K.hess and pre.values.jac is K.jac and pre.values.dc is K.dc
    delta, dxp = pre.delta.cpu().numpy(), pre.values.dx.cpu().numpy()
    print("%s: tries %s delta %s" % (name, pre.tries.cpu().numpy().tolist(), delta.tolist()))
    assert np.array_equal(bits(dxp[:, :NXK * horizon]), bits(d["dx"][:, :NXK * horizon] + np.repeat(delta, NXK, axis=1)))
    assert np.array_equal(bits(dxp[:, NXK * horizon:]), bits(d["dx"][:, NXK * horizon:])) and dxp.shape[1] == NXK * horizon + 6
    assert np.array_equal(K.dx.cpu().numpy(), d["dx"])                           # the operator it was built from keeps its own dx
    refs = []
    for b in range(B):
        what = "%s convexify b=%d" % (name, b)
        ref = emu.block_ladder(d["hess"][b], d["dx"][b], FLOOR, 1e-4, 8.0, 16)
        assert_ladder_equals(pre, ref, b, what)
        assert np.array_equal(bits(emu.convexified_dx(d["dx"][b], ref.delta)), bits(dxp[b]))
        diag = emu.diagonal_preconditioner(d["hess"][b], d["jac"][b], dxp[b], d["dc"][b], FLOOR)
        assert np.array_equal(bits(pre.top_diagonal[b].cpu().numpy()), bits(diag.top)) and np.array_equal(bits(pre.bottom[b].cpu().numpy()), bits(diag.bottom)), what
        app = emu.block_apply(ref, (diag.top, diag.bottom), d["bt"][b], d["bb"][b])
        assert np.array_equal(bits(zt[b].cpu().numpy()), bits(app.top)) and np.array_equal(bits(zb[b].cpu().numpy()), bits(app.bottom)), what
        refs.append(emu.block_solve(d["hess"][b], d["jac"][b], d["bt"][b], d["bb"][b], ref, (diag.top, diag.bottom), dx=dxp[b], dc=d["dc"][b], rtol=1e-8, maxiter=12))
    z = pre.values.solve(dev(d["bt"]), dev(d["bb"]), rtol=1e-8, maxiter=12, minv=pre, check_every=5)
    torch.cuda.synchronize()
    top, bottom, its, res, status = (a.cpu().numpy() for a in z)
    for b, ref in enumerate(refs):
        print("%s b=%d: status %d / %d, iterations %d / %d, residual %.3e / %.3e (device / emulation)" % (name, b, status[b], ref.status, its[b], ref.iterations, res[b], ref.residual))
        assert (int(status[b]), int(its[b])) == (ref.status, ref.iterations), (name, b)
        assert bits(res[b:b + 1])[0] == bits([ref.residual])[0], (name, b)
        assert np.array_equal(bits(top[b]), bits(ref.top)) and np.array_equal(bits(bottom[b]), bits(ref.bottom)), (name, b)


def test_convexify_without_diagonals_and_with_an_exhausted_ladder_is_not_quasi_definite(model):
    import torch
    nlp, K, d = real(model, "periodic", 4)
    bare = K.with_diagonals(None, None).convexify(floor=FLOOR)                   # dx None counts as zeros: the globals are 0, dc is missing
    short = K.convexify(delta_init=1e-300, max_tries=1, floor=FLOOR)
    torch.cuda.synchronize()
    assert bare.quasi_definite.cpu().numpy().tolist() == [False] * B and bool((bare.status == 0).all())
    dxp = bare.values.dx.cpu().numpy()
    assert np.array_equal(bits(dxp[:, :NXK * 4]), bits(np.repeat(bare.delta.cpu().numpy(), NXK, axis=1))) and np.all(bits(dxp[:, NXK * 4:]) == 0)
    assert short.quasi_definite.cpu().numpy().tolist()[0] is False and int(short.status[0, 0]) == 3


# ---- 3. handles the block entry points do not serve ------------------------------------------------------------------------------------------
def test_a_multi_device_and_a_shard_handle_are_unsupported_as_for_the_factor_launch(model):
    import torch
    from hippopt_amd.hipnlp import HipNlp, HipNlpError
    nlp, K, d = real(model, "periodic", 4)
    out = Arrays(nlp, 4)
    st = MAKERS["periodic"](4, model)
    stream = torch.cuda.current_stream().cuda_stream
    for other, word in ((HipNlp(st, model, devices=[0, 0]), "multi-device"), (HipNlp(st, model, knot_begin=0, knot_end=2), "shard")):
        with pytest.raises(HipNlpError) as factor:
            other.kkt_block_factor_device(K.hess.data_ptr(), *(t.data_ptr() for t in out.six()), floor=FLOOR, stream=stream)
        with pytest.raises(HipNlpError) as ladder:
            other.kkt_block_ladder_device(K.hess.data_ptr(), *(t.data_ptr() for t in out.six()), out.delta.data_ptr(), out.tries.data_ptr(), floor=FLOOR, delta_init=1e-4,
                                          kappa=8.0, max_tries=16, stream=stream)
        assert factor.value.code == ladder.value.code == E_UNSUPPORTED and word in str(ladder.value) and "hipnlp_kkt_block_ladder_device" in str(ladder.value)
    torch.cuda.synchronize()
    assert bool((out.tries == -77).all()) and bool((out.status == -77).all())     # nothing was launched
