"""The C-ABI, the ctypes binding and the torch entry points of the pose finder's KKT chain (hipnlp_pose_kkt_times_device,
hipnlp_pose_kkt_diag_precond_device, hipnlp_pose_kkt_minres_device; HipPose.kkt_*_device; hippopt_amd.autograd.PoseNLP.kkt and
PoseKKTValues): declarations, exports, and the Python-level argument checks, which all happen before anything touches a device.  CPU only."""
import inspect
import os
import re

import pytest

from hippopt_amd import _abi, autograd, hipnlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMETERS = {"hipnlp_pose_kkt_times_device": 10, "hipnlp_pose_kkt_diag_precond_device": 9, "hipnlp_pose_kkt_minres_device": 19}


@pytest.mark.parametrize("name", sorted(PARAMETERS))
def test_entry_point_is_declared_exported_and_bound(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(\s*hipnlp_pose_handle\s*\*([^;]*)\)\s*;" % name, src)
    assert decl, "not declared in include/hipnlp.h"
    assert decl.group(1).count(",") == PARAMETERS[name] - 1
    assert name in hipnlp.EXPORTS
    fn = getattr(hipnlp.load_library(), name)     # (AttributeError: the built library does not export it)
    assert fn.argtypes is not None and len(fn.argtypes) == PARAMETERS[name]


def test_abi_version_is_unchanged():
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (no structure of include/hipnlp.h changed)


def test_a_missing_handle_is_an_invalid_argument():
    lib = hipnlp.load_library()
    assert lib.hipnlp_pose_kkt_times_device(*([None] * 10)) == _abi.E_INVALID
    assert lib.hipnlp_pose_kkt_diag_precond_device(*([None] * 7 + [1e-10, None])) == _abi.E_INVALID
    assert lib.hipnlp_pose_kkt_minres_device(*([None] * 14 + [0, 1e-10, 1e-8, 10, None])) == _abi.E_INVALID


def test_binding_and_autograd_surface():
    p = inspect.signature(hipnlp.HipPose.kkt_times_device).parameters
    assert list(p) == ["self", "hess_values_ptr", "jac_values_ptr", "v_ptr", "w_ptr", "top_ptr", "bottom_ptr", "dx_ptr", "dc_ptr", "stream"]
    p = inspect.signature(hipnlp.HipPose.kkt_diag_precond_device).parameters
    assert list(p) == ["self", "hess_values_ptr", "jac_values_ptr", "minv_top_ptr", "minv_bottom_ptr", "dx_ptr", "dc_ptr", "floor", "stream"]
    p = inspect.signature(hipnlp.HipPose.kkt_minres_device).parameters
    assert list(p)[-9:] == ["dx_ptr", "dc_ptr", "minv_top_ptr", "minv_bottom_ptr", "build_diagonal", "floor", "rtol", "max_iterations", "stream"]
    assert "check_every" not in p and not hasattr(hipnlp.HipPose, "kkt_minres_reserve")       # one launch: no workspace, nothing to wait for
    s = inspect.signature(autograd.PoseKKTValues.solve).parameters
    assert list(s) == ["self", "rhs_top", "rhs_bottom", "rtol", "maxiter", "minv", "floor"]
    assert (s["rtol"].default, s["maxiter"].default, s["minv"].default) == (1e-8, 400, None)
    q = inspect.signature(autograd.PoseKKTValues.diagonal_preconditioner).parameters
    assert list(q) == ["self", "floor"] and q["floor"].default == 1e-10
    assert list(inspect.signature(autograd.PoseNLP.kkt).parameters) == ["self", "x", "sigma", "lam", "dx", "dc"]
    for name in PARAMETERS:
        assert name in autograd.__doc__ or name in autograd.PoseKKTValues.solve.__doc__ + autograd.PoseKKTValues.matvec.__doc__ + autograd.PoseKKTValues.diagonal_preconditioner.__doc__


class _Engine:
    """stands in for a pose handle: records the calls a valid request makes"""
    nnz = 5

    def __init__(self):
        self.calls = []

    def kkt_times_device(self, *args, **kw):
        self.calls.append(("times", args, kw))

    def kkt_diag_precond_device(self, *args, **kw):
        self.calls.append(("diag", args, kw))

    def kkt_minres_device(self, *args, **kw):
        self.calls.append(("minres", args, kw))


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


def test_the_value_runs_and_the_diagonals_are_checked():
    import torch
    nlp = _Nlp()
    autograd.PoseKKTValues(nlp, _z(2, 7), _z(2, 5), _z(2, 4), _z(2, 3))
    for hess, jac, dx, dc, err in ((_z(2, 6), _z(2, 5), None, None, ValueError), (_z(2, 7), _z(3, 5), None, None, ValueError), (_z(2, 7), _z(2, 5), _z(2, 3), None, ValueError),
                                   (_z(2, 7), _z(2, 5), None, _z(2, 4), ValueError), (_z(2, 7).float(), _z(2, 5), None, None, TypeError),
                                   (_z(2, 7).numpy(), _z(2, 5), None, None, TypeError), (_z(2, 7), _z(5, 2).t(), None, None, ValueError)):
        with pytest.raises(err):
            autograd.PoseKKTValues(nlp, hess, jac, dx, dc)
    assert nlp.engine.calls == [] and torch.float64 == _z(1).dtype


def test_matvec_and_diagonal_preconditioner_check_their_arguments_before_any_launch():
    nlp = _Nlp()
    K = autograd.PoseKKTValues(nlp, _z(2, 7), _z(2, 5), _z(2, 4), None)
    for v, w in ((_z(2, 3), _z(2, 3)), (_z(2, 4), _z(2, 4)), (_z(2, 4).float(), _z(2, 3))):
        with pytest.raises((ValueError, TypeError)):
            K.matvec(v, w)
    for bad in (0.0, -1e-10, float("nan"), float("inf"), "1e-10", None, True):
        with pytest.raises(ValueError):
            K.diagonal_preconditioner(floor=bad)
    assert nlp.engine.calls == []
    v, w = _z(2, 4), _z(2, 3)
    top, bottom = K.matvec(v, w)
    mt, mb = K.diagonal_preconditioner(floor=0.5)
    (k0, a0, kw0), (k1, a1, kw1) = nlp.engine.calls
    assert (k0, a0) == ("times", (K.hess.data_ptr(), K.jac.data_ptr(), v.data_ptr(), w.data_ptr(), top.data_ptr(), bottom.data_ptr()))
    assert kw0 == dict(dx_ptr=K.dx.data_ptr(), dc_ptr=0, stream=0)
    assert (k1, a1) == ("diag", (K.hess.data_ptr(), K.jac.data_ptr(), mt.data_ptr(), mb.data_ptr())) and kw1 == dict(dx_ptr=K.dx.data_ptr(), dc_ptr=0, floor=0.5, stream=0)
    assert top.shape == mt.shape == (2, 4) and bottom.shape == mb.shape == (2, 3)
    K2 = K.with_diagonals(None, _z(2, 3))
    assert K2.hess is K.hess and K2.jac is K.jac and K2.dx is None and K2.dc is not None and len(nlp.engine.calls) == 2       # no launch


def test_solve_checks_its_arguments_before_any_launch():
    import torch
    nlp = _Nlp()
    K = autograd.PoseKKTValues(nlp, _z(2, 7), _z(2, 5), _z(2, 4), _z(2, 3))
    bt, bb = _z(2, 4), _z(2, 3)
    for kw, err in ((dict(rtol=-1.0), ValueError), (dict(rtol="x"), ValueError), (dict(maxiter=-1), ValueError), (dict(maxiter=4097), ValueError), (dict(maxiter=2.0), ValueError),
                    (dict(maxiter=True), ValueError), (dict(floor=0.0), ValueError), (dict(floor=float("inf")), ValueError), (dict(minv="jacobi"), ValueError),
                    (dict(minv=_z(2, 4)), TypeError), (dict(minv=(_z(2, 4),)), TypeError), (dict(minv=(_z(2, 3), _z(2, 3))), ValueError), (dict(minv=(_z(2, 4), _z(2, 4))), ValueError)):
        with pytest.raises(err):
            K.solve(bt, bb, **kw)
    with pytest.raises(ValueError):
        K.solve(_z(2, 3), bb)
    with pytest.raises(ValueError):
        K.solve(bt, _z(2, 4))
    assert nlp.engine.calls == []
    z = K.solve(bt, bb)
    assert isinstance(z, autograd.KKTSolution) and z.top.shape == (2, 4) and z.bottom.shape == (2, 3)
    assert z.iterations.dtype == z.status.dtype == torch.int32 and z.iterations.shape == z.status.shape == z.residual.shape == (2,)
    mt, mb = _z(2, 4) + 1.0, _z(2, 3) + 1.0
    K.solve(bt, bb, rtol=0.0, maxiter=4096, minv=(mt, mb))
    K.solve(bt, bb, minv="diagonal", floor=1e-300)
    (_, a0, kw0), (_, _, kw1), (_, _, kw2) = nlp.engine.calls
    assert a0[:4] == (K.hess.data_ptr(), K.jac.data_ptr(), bt.data_ptr(), bb.data_ptr()) and a0[4:6] == (z.top.data_ptr(), z.bottom.data_ptr())
    assert kw0 == dict(dx_ptr=K.dx.data_ptr(), dc_ptr=K.dc.data_ptr(), minv_top_ptr=0, minv_bottom_ptr=0, build_diagonal=False, floor=1e-10, rtol=1e-8, max_iterations=400, stream=0)
    assert (kw1["minv_top_ptr"], kw1["minv_bottom_ptr"], kw1["build_diagonal"], kw1["max_iterations"], kw1["rtol"]) == (mt.data_ptr(), mb.data_ptr(), False, 4096, 0.0)
    assert (kw2["minv_top_ptr"], kw2["minv_bottom_ptr"], kw2["build_diagonal"], kw2["floor"]) == (0, 0, True, 1e-300)
