"""The copy-out of the two-workgroups-per-knot kernels (SPLIT instantiations of hipnlp_knot_kernel) on the GPU.  Their final stores of
jac g, g and grad f are written through the L2 (`sc1`, inline assembly with 32-bit offsets from a uniform base) instead of left dirty in
it — the only thing that differs from the one-workgroup kernel's copy-out.  Addressing only (the reference's rows and costs are unchanged:
/root/reference/src/hippopt/turnkey_planners/humanoid_kinodynamic/planner.py:124-176): f, grad f, g, jac g and the cost terms are, bit
for bit, those of the one-workgroup kernel (the diagnostic build's HIPNLP_SPLIT=0); nothing is left unwritten, nothing is written
outside the arrays, and a non-finite value raises the same flag.  Horizons of 2 (no interior knot), 3 (one) and 4; the file keeps the
name the packed copy-out tables gave it, which were built, measured and not adopted (profiles/r10_split_packed_copy_out.txt)."""
import ctypes as C

import numpy as np
import pytest

from hippopt_amd.kinodyn_settings import periodic_step_settings, single_step_settings, stairs_settings
from hippopt_amd.synthetic import make_workload, place_on_step_flanks

pytestmark = pytest.mark.gpu

CANARY = 64
CANARY_VALUE = -7.25e77
MAKERS = {"periodic": periodic_step_settings, "single_step": single_step_settings, "stairs": stairs_settings}


def run(st, model, x, p, batch, vary_first, split):
    """three eval_device calls of a diagnostic-build handle into NaN-filled arrays between canaries:
    (workgroups per knot of the last launch, [f, grad, g, jac, cost terms], non-finite flags)"""
    import torch
    from diag_lib import diag_library, diag_overrides
    from hippopt_amd.hipnlp import HipNlp
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(x).to(dev)
    with diag_overrides(HIPNLP_SPLIT=split):
        eng = HipNlp(st, model, batch=batch, jac_varying_first=vary_first, library=diag_library())
    eng.set_params(p)
    sizes = (1, eng.n, eng.m, eng.nnz)
    bufs = [torch.full((batch * k + 2 * CANARY,), CANARY_VALUE, dtype=torch.float64, device=dev) for k in sizes]
    for t in bufs:
        t[CANARY:-CANARY] = float("nan")
    for _ in range(3):      # (the jac buffer of a varying-first handle receives its constants at first sight, the varying runs ever after)
        eng.eval_device(xd.data_ptr(), *[t.data_ptr() + 8 * CANARY for t in bufs])
    wgs, raised = C.c_int(), np.zeros(batch, np.int32)      # (diagnostic build only: hipnlp_debug_last_launch)
    eng.lib.hipnlp_debug_last_launch.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int32)]
    assert eng.lib.hipnlp_debug_last_launch(eng.h, C.byref(wgs), raised.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    outs = []
    for t, name in zip(bufs, ("f", "grad", "g", "jac")):
        h = t.cpu().numpy()
        assert np.all(h[:CANARY] == CANARY_VALUE) and np.all(h[-CANARY:] == CANARY_VALUE), ("canary of " + name, split)
        outs.append(h[CANARY:-CANARY].reshape(batch, -1).copy())
    outs.append(eng.cost_terms()[1])
    eng.close()
    return wgs.value, outs, raised.astype(bool)


@pytest.mark.parametrize("horizon", [2, 3, 4])
@pytest.mark.parametrize("maker", sorted(MAKERS))
def test_written_through_copy_out_gives_the_one_workgroup_bits(model, maker, horizon):
    st = MAKERS[maker](horizon, model)
    for batch in (1, 2):
        x, p = make_workload(st, model, batch=batch, seed=9200 + 10 * horizon + batch)
        if st.terrain != 0:
            place_on_step_flanks(x[:1], st, seed=horizon)
        for vary_first in (False, True):
            wgs2, two, flags2 = run(st, model, x, p, batch, vary_first, 1)
            wgs1, one, flags1 = run(st, model, x, p, batch, vary_first, 0)
            assert (wgs2, wgs1) == (2, 1), "the launch under test did not run two workgroups per knot"
            for name, a, b in zip(("f", "grad", "g", "jac", "cost terms"), two, one):
                assert not np.isnan(a).any(), (name, batch, vary_first)
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, batch, vary_first)
            assert not flags2.any() and not flags1.any()


@pytest.mark.parametrize("maker,horizon", [("periodic", 3), ("stairs", 4)])
def test_an_infinite_joint_velocity_raises_the_same_flag(model, maker, horizon):
    st = MAKERS[maker](horizon, model)
    x, p = make_workload(st, model, batch=2, seed=9300 + horizon)
    x[1, 189 * 1 + 134 + 5] = np.inf        # a joint velocity of knot 1, second trajectory only
    wgs2, two, flags2 = run(st, model, x, p, 2, False, 1)
    wgs1, one, flags1 = run(st, model, x, p, 2, False, 0)
    assert (wgs2, wgs1) == (2, 1)
    assert flags1.tolist() == [False, True] and flags2.tolist() == flags1.tolist()
    for name, a, b in zip(("f", "grad", "g", "jac", "cost terms"), two, one):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), name       # (the non-finite values included, where they are)
        assert np.isfinite(a[0]).all(), name
