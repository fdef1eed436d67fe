"""The C-ABI, the ctypes binding and the torch entry points of the pose finder's dense L D L^T (hipnlp_pose_kkt_ldl_doubles,
hipnlp_pose_kkt_ldl_device, hipnlp_pose_kkt_ldl_solve_device; HipPose.kkt_ldl_*; hippopt_amd.autograd.PoseKKTValues.factor / solve_direct and
PoseKKTFactor): declarations, exports, every refusal of the two entry points — pose_ldl.h's pl_factor_call_error / pl_solve_call_error,
the one text the library calls before it touches a device, here through the emulation — and the Python-level argument checks.  CPU only."""
import inspect
import os
import re

import pytest

import pose_ldl_emu_lib as pl
from hippopt_amd import _abi, autograd, hipnlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMETERS = {"hipnlp_pose_kkt_ldl_doubles": 1, "hipnlp_pose_kkt_ldl_device": 20, "hipnlp_pose_kkt_ldl_solve_device": 9}


@pytest.mark.parametrize("name", sorted(PARAMETERS))
def test_entry_point_is_declared_exported_and_bound(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(\s*(?:const\s+)?hipnlp_pose_handle\s*\*([^;]*)\)\s*;" % name, src)
    assert decl, "not declared in include/hipnlp.h"
    assert decl.group(1).count(",") == PARAMETERS[name] - 1
    assert name in hipnlp.EXPORTS
    fn = getattr(hipnlp.load_library(), name)     # (AttributeError: the built library does not export it)
    assert fn.argtypes is not None and len(fn.argtypes) == PARAMETERS[name]


def test_abi_version_is_unchanged():
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (no structure of include/hipnlp.h changed)


def test_a_missing_handle_is_an_invalid_argument():
    lib = hipnlp.load_library()
    assert lib.hipnlp_pose_kkt_ldl_doubles(None) == _abi.E_INVALID
    assert lib.hipnlp_pose_kkt_ldl_device(*([None] * 5 + [0] + [None] * 8 + [0.0, 0.0, 0] + [None] * 3)) == _abi.E_INVALID
    assert lib.hipnlp_pose_kkt_ldl_solve_device(*([None] * 3 + [1] + [None] * 5)) == _abi.E_INVALID


def test_the_library_refuses_by_the_text_the_emulation_states():
    src = open(os.path.join(ROOT, "hippopt_amd", "csrc", "hipnlp_pose.hip")).read()
    body = src[src.index("int hipnlp_pose_kkt_ldl_device("):src.index("int hipnlp_pose_cost_terms(")]
    assert body.count("pl_factor_call_error(") == 1 and body.count("pl_solve_call_error(") == 1 and body.count("return HIPNLP_E_INVALID;") == 4
    for call in ("pl_factor_call_error(", "pl_solve_call_error("):                 # the refusal stands in front of the launch
        assert body.index(call) < body.index("pose_ldl_launch(", body.index(call))


def test_every_refusal_of_the_factorisation_without_a_device():
    ok = dict(nrhs=1)
    assert pl.call_error("factor", **ok) is None
    assert pl.call_error("factor", nrhs=0, rhs_top=False, rhs_bottom=False, sol_top=False, sol_bottom=False, factor=False, pivots=False) is None      # the inertia-only call
    assert pl.call_error("factor", nrhs=8, max_tries=16, delta_init=1e-300, kappa=1.0000001) is None
    assert pl.call_error("factor", max_tries=0, delta_init=float("nan"), kappa=-1.0) is None                    # no ladder: its numbers are not read
    for k in ("hess", "jac", "inertia", "status"):
        assert pl.call_error("factor", **{k: False}), k
    for k in ("rhs_top", "rhs_bottom", "sol_top", "sol_bottom"):
        assert pl.call_error("factor", **{k: False}), k
    for nrhs in (-1, 9):
        assert pl.call_error("factor", nrhs=nrhs)
    assert pl.call_error("factor", factor=False) and pl.call_error("factor", pivots=False)
    for max_tries in (-1, 17):
        assert pl.call_error("factor", max_tries=max_tries, delta_init=1e-4, kappa=8.0)
    for delta_init in (0.0, -1e-4, float("nan"), float("inf")):
        assert pl.call_error("factor", max_tries=1, delta_init=delta_init, kappa=8.0), delta_init
    for kappa in (1.0, 0.5, float("nan"), float("inf")):
        assert pl.call_error("factor", max_tries=1, delta_init=1e-4, kappa=kappa), kappa


def test_every_refusal_of_the_stored_factor_solve_without_a_device():
    assert pl.call_error("solve", nrhs=1) is None and pl.call_error("solve", nrhs=8) is None
    for k in ("factor", "pivots", "rhs_top", "rhs_bottom", "sol_top", "sol_bottom"):
        assert pl.call_error("solve", **{k: False}), k
    for nrhs in (0, -1, 9):
        assert pl.call_error("solve", nrhs=nrhs)


def test_binding_and_autograd_surface():
    p = inspect.signature(hipnlp.HipPose.kkt_ldl_device).parameters
    assert list(p) == ["self", "hess_values_ptr", "jac_values_ptr", "inertia_ptr", "status_ptr", "dx_ptr", "dc_ptr", "nrhs", "rhs_top_ptr", "rhs_bottom_ptr", "sol_top_ptr",
                       "sol_bottom_ptr", "delta_ptr", "tries_ptr", "delta_init", "kappa", "max_tries", "factor_ptr", "pivots_ptr", "stream"]
    p = inspect.signature(hipnlp.HipPose.kkt_ldl_solve_device).parameters
    assert list(p) == ["self", "factor_ptr", "pivots_ptr", "nrhs", "rhs_top_ptr", "rhs_bottom_ptr", "sol_top_ptr", "sol_bottom_ptr", "stream"]
    assert list(inspect.signature(hipnlp.HipPose.kkt_ldl_doubles).parameters) == ["self"]
    f = inspect.signature(autograd.PoseKKTValues.factor).parameters
    assert list(f) == ["self", "delta_init", "kappa", "max_tries"] and (f["delta_init"].default, f["kappa"].default, f["max_tries"].default) == (None, 8.0, 0)
    assert list(inspect.signature(autograd.PoseKKTValues.solve_direct).parameters) == ["self", "rhs_top", "rhs_bottom", "delta_init", "kappa", "max_tries"]
    s = inspect.signature(autograd.PoseKKTFactor.solve).parameters
    assert list(s) == ["self", "rhs_top", "rhs_bottom", "refine"] and s["refine"].default == 0
    assert "delta = 0" in autograd.PoseKKTFactor.solve.__doc__ and "dx + delta" in autograd.PoseKKTFactor.solve.__doc__
    for name in ("hipnlp_pose_kkt_ldl_device", "hipnlp_pose_kkt_ldl_solve_device"):
        assert name in autograd.PoseKKTValues.factor.__doc__ + autograd.PoseKKTFactor.solve.__doc__


class _Engine:
    """stands in for a pose handle: records the calls a valid request makes"""
    nnz = 5

    def __init__(self):
        self.calls = []

    def kkt_ldl_doubles(self):
        return 28

    def kkt_times_device(self, *args, **kw):
        self.calls.append(("times", args, kw))

    def kkt_ldl_device(self, *args, **kw):
        self.calls.append(("ldl", args, kw))

    def kkt_ldl_solve_device(self, *args, **kw):
        self.calls.append(("ldl_solve", args, kw))


class _Nlp(autograd._DeviceNLP):
    """a _DeviceNLP on the CPU device: _check runs as it does on a GPU, the launches go to the recording engine"""
    batch, n, m, device_index, hess_nnz = 2, 4, 3, 0, 7

    def __init__(self):
        self.engine = _Engine()

    @property
    def device(self):
        import torch
        return torch.device("cpu")

    def _on_current_stream(self, launch):
        launch(0)


def _z(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.float64)


def test_factor_and_solve_direct_check_their_arguments_before_any_launch():
    import torch
    nlp = _Nlp()
    K = autograd.PoseKKTValues(nlp, _z(2, 7), _z(2, 5), _z(2, 4), None)
    for kw in (dict(max_tries=-1), dict(max_tries=17), dict(max_tries=1.0), dict(max_tries=True), dict(max_tries=1), dict(max_tries=1, delta_init=0.0),
               dict(max_tries=1, delta_init=float("inf")), dict(max_tries=1, delta_init="x"), dict(max_tries=1, delta_init=1e-4, kappa=1.0),
               dict(max_tries=1, delta_init=1e-4, kappa=float("nan"))):
        with pytest.raises(ValueError):
            K.factor(**kw)
        with pytest.raises(ValueError):
            K.solve_direct(_z(2, 4), _z(2, 3), **kw)
    for bt, bb in ((_z(2, 3), _z(2, 3)), (_z(2, 4), _z(2, 4)), (_z(2, 9, 4), _z(2, 9, 3)), (_z(2, 2, 4), _z(2, 3, 3)), (_z(4), _z(3)), (_z(2, 4).float(), _z(2, 3))):
        with pytest.raises((ValueError, TypeError)):
            K.solve_direct(bt, bb)
    assert nlp.engine.calls == []
    F = K.factor(delta_init=1e-4, max_tries=5)
    assert isinstance(F, autograd.PoseKKTFactor) and F.factor.shape == (2, 28) and F.pivots.shape == (2, 7) and F.pivots.dtype == torch.int32
    assert F.inertia.shape == (2, 3) and F.inertia.dtype == F.status.dtype == F.tries.dtype == torch.int32 and F.delta.dtype == torch.float64
    (k0, a0, kw0), = nlp.engine.calls
    assert k0 == "ldl" and a0 == (K.hess.data_ptr(), K.jac.data_ptr(), F.inertia.data_ptr(), F.status.data_ptr())
    assert kw0 == dict(nrhs=0, rhs_top_ptr=0, rhs_bottom_ptr=0, sol_top_ptr=0, sol_bottom_ptr=0, delta_ptr=F.delta.data_ptr(), tries_ptr=F.tries.data_ptr(), delta_init=1e-4, kappa=8.0,
                       max_tries=5, factor_ptr=F.factor.data_ptr(), pivots_ptr=F.pivots.data_ptr(), stream=0, dx_ptr=K.dx.data_ptr(), dc_ptr=0)
    bt, bb = _z(2, 3, 4), _z(2, 3, 3)
    top, bottom, inertia, status = K.solve_direct(bt, bb)
    kw1 = nlp.engine.calls[1][2]
    assert top.shape == bt.shape and bottom.shape == bb.shape and (kw1["nrhs"], kw1["factor_ptr"], kw1["pivots_ptr"], kw1["max_tries"]) == (3, 0, 0, 0)
    assert (kw1["rhs_top_ptr"], kw1["sol_top_ptr"], kw1["sol_bottom_ptr"]) == (bt.data_ptr(), top.data_ptr(), bottom.data_ptr())


def test_the_factor_solves_and_refines_with_existing_launches():
    nlp = _Nlp()
    K = autograd.PoseKKTValues(nlp, _z(2, 7), _z(2, 5), None, _z(2, 3))
    F = K.factor()
    bt, bb = _z(2, 4), _z(2, 3)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            F.solve(bt, bb, refine=bad)
    with pytest.raises(ValueError):
        F.solve(_z(2, 4), _z(2, 4))
    assert [c[0] for c in nlp.engine.calls] == ["ldl"]
    top, bottom = F.solve(bt, bb)
    assert top.shape == (2, 4) and bottom.shape == (2, 3) and [c[0] for c in nlp.engine.calls] == ["ldl", "ldl_solve"]
    assert nlp.engine.calls[1][1][:5] == (F.factor.data_ptr(), F.pivots.data_ptr(), 1, bt.data_ptr(), bb.data_ptr())
    F.solve(bt, bb, refine=2)
    assert [c[0] for c in nlp.engine.calls[2:]] == ["ldl_solve", "times", "ldl_solve", "times", "ldl_solve"]
    assert nlp.engine.calls[3][2]["dx_ptr"] == 0                                   # no ladder: the values' own operator
    del nlp.engine.calls[:]
    F = K.factor(delta_init=1e-4, max_tries=3)
    F.solve(_z(2, 2, 4), _z(2, 2, 3), refine=1)
    assert [c[0] for c in nlp.engine.calls] == ["ldl", "ldl_solve", "times", "times", "ldl_solve"]
    assert nlp.engine.calls[2][2]["dx_ptr"] != 0 and nlp.engine.calls[1][1][2] == 2   # a ladder: the refinement runs against dx + delta
