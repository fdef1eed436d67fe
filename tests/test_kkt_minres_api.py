"""The C-ABI, the ctypes binding and the torch entry point of the device-resident MINRES solve on the KKT operator
(hipnlp_kkt_minres_device, hipnlp_kkt_minres_reserve; HipNlp.kkt_minres_device; hippopt_amd.autograd.KKTValues.solve): declarations,
exports, and the argument checks of KKTValues.solve, which all happen before anything touches a device.  CPU only."""
import inspect
import os
import re

import pytest

from hippopt_amd import _abi, autograd, hipnlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, RESERVE = "hipnlp_kkt_minres_device", "hipnlp_kkt_minres_reserve"


def test_entry_points_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(\s*hipnlp_handle\s*\*([^;]*)\)\s*;" % NAME, src)
    assert decl, "not declared in include/hipnlp.h"
    assert decl.group(1).count(",") == 17         # handle + 10 pointers + rtol, max_iterations, check_every + 3 outputs + stream: 18 parameters
    assert re.search(r"\bint\s+%s\s*\(\s*hipnlp_handle\s*\*\s*h\s*,\s*int64_t\s*\*\s*bytes_out\s*\)\s*;" % RESERVE, src)
    lib = hipnlp.load_library()
    for name, count in ((NAME, 18), (RESERVE, 2)):
        assert name in hipnlp.EXPORTS
        fn = getattr(lib, name)                   # (AttributeError: the built library does not export it)
        assert fn.argtypes is not None and len(fn.argtypes) == count


def test_abi_version_is_unchanged():
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (the descriptor did not change)


def test_a_missing_handle_is_an_invalid_argument():
    lib = hipnlp.load_library()
    assert lib.hipnlp_kkt_minres_device(*([None] * 11 + [1e-8, 10, 0] + [None] * 4)) == _abi.E_INVALID
    assert lib.hipnlp_kkt_minres_reserve(None, None) == _abi.E_INVALID


def test_binding_and_autograd_surface():
    p = inspect.signature(hipnlp.HipNlp.kkt_minres_device).parameters
    assert list(p)[:10] == ["self", "hess_values_ptr", "jac_values_ptr", "rhs_top_ptr", "rhs_bottom_ptr", "sol_top_ptr", "sol_bottom_ptr", "iterations_ptr", "residual_ptr",
                            "status_ptr"]
    assert all(p[k].default == 0 for k in ("dx_ptr", "dc_ptr", "minv_top_ptr", "minv_bottom_ptr", "stream"))
    assert callable(hipnlp.HipNlp.kkt_minres_reserve)
    q = inspect.signature(autograd.KKTValues.solve).parameters
    assert list(q) == ["self", "rhs_top", "rhs_bottom", "rtol", "maxiter", "minv", "check_every"]
    assert (q["rtol"].default, q["maxiter"].default, q["minv"].default, q["check_every"].default) == (1e-8, 200, None, 16)
    assert autograd.KKTSolution._fields == ("top", "bottom", "iterations", "residual", "status")
    assert "hipnlp_kkt_minres_device" in autograd.__doc__ and "No convergence is promised" in " ".join(autograd.KKTValues.solve.__doc__.split())


class _Engine:
    """stands in for a handle: records the one call a valid solve makes"""

    def __init__(self):
        self.calls = []

    def hess_nnz(self):
        return 7

    nnz = 5

    def kkt_minres_device(self, *args, **kw):
        self.calls.append((args, kw))


class _Nlp(autograd._DeviceNLP):
    """a _DeviceNLP on the CPU device: _check runs as it does on a GPU, the launch goes to the recording engine"""
    batch, n, m, device_index = 2, 4, 3, 0

    def __init__(self):
        self.engine = _Engine()

    @property
    def device(self):
        import torch
        return torch.device("cpu")

    def _on_current_stream(self, launch):
        launch(0)


def _operator():
    import torch
    nlp = _Nlp()
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    return nlp, autograd.KKTValues(nlp, z(2, 7), z(2, 5), z(2, 4), z(2, 3)), z


def test_solve_checks_its_arguments_before_any_launch():
    import torch
    nlp, K, z = _operator()
    bt, bb = z(2, 4), z(2, 3)
    wide = z(2, 8)
    for exc, t in ((TypeError, bt.float()), (TypeError, [0.0] * 8), (ValueError, bt[:1]), (ValueError, z(2, 5)), (ValueError, wide[:, ::2])):
        with pytest.raises(exc):
            K.solve(t, bb)
        with pytest.raises(exc):
            K.solve(bt, bb, minv=(t, bb))
    for exc, t in ((TypeError, bb.float()), (ValueError, bb[:1]), (ValueError, z(2, 4))):
        with pytest.raises(exc):
            K.solve(bt, t)
        with pytest.raises(exc):
            K.solve(bt, bb, minv=(bt, t))
    for bad in (bt, (bt,), (bt, bb, bb)):
        with pytest.raises(TypeError):
            K.solve(bt, bb, minv=bad)
    for kw in (dict(rtol=-1e-8), dict(rtol=float("nan")), dict(rtol="1e-8"), dict(maxiter=-1), dict(maxiter=2.5), dict(maxiter=True), dict(check_every=-1), dict(check_every=1.0)):
        with pytest.raises(ValueError):
            K.solve(bt, bb, **kw)
    assert nlp.engine.calls == []                                            # nothing reached the engine
    sol = K.solve(bt, bb, rtol=1e-6, maxiter=9, minv=(bt, bb), check_every=0)
    assert len(nlp.engine.calls) == 1
    args, kw = nlp.engine.calls[0]
    assert args[:4] == (K.hess.data_ptr(), K.jac.data_ptr(), bt.data_ptr(), bb.data_ptr())
    assert args[4:] == (sol.top.data_ptr(), sol.bottom.data_ptr(), sol.iterations.data_ptr(), sol.residual.data_ptr(), sol.status.data_ptr())
    assert kw == dict(dx_ptr=K.dx.data_ptr(), dc_ptr=K.dc.data_ptr(), minv_top_ptr=bt.data_ptr(), minv_bottom_ptr=bb.data_ptr(), rtol=1e-6, max_iterations=9, check_every=0, stream=0)
    assert sol.top.shape == (2, 4) and sol.bottom.shape == (2, 3) and sol.iterations.dtype == torch.int32 and sol.status.dtype == torch.int32 and sol.residual.shape == (2,)
    K.with_diagonals(None, None).solve(bt, bb)
    assert nlp.engine.calls[1][1]["dx_ptr"] == 0 and nlp.engine.calls[1][1]["minv_top_ptr"] == 0 and nlp.engine.calls[1][1]["check_every"] == 16
