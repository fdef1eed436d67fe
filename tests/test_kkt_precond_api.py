"""The C-ABI, the ctypes binding and the torch entry point of the device-built diagonal preconditioner of the KKT solve
(hipnlp_kkt_diag_precond_device; HipNlp.kkt_diag_precond_device; hippopt_amd.autograd.KKTValues.diagonal_preconditioner): declarations,
exports, and the argument checks of diagonal_preconditioner, which all happen before anything touches a device.  (A floor that is not a
finite number > 0 on a live handle: tests/test_gpu_kkt_precond.py.)  CPU only."""
import inspect
import os
import re

import pytest

from hippopt_amd import _abi, autograd, hipnlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hipnlp_kkt_diag_precond_device"


def test_entry_point_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(\s*hipnlp_handle\s*\*([^;]*)\)\s*;" % NAME, src)
    assert decl, "not declared in include/hipnlp.h"
    assert decl.group(1).count(",") == 8          # handle + 4 inputs + floor + 2 outputs + stream: 9 parameters
    assert re.search(r"\bdouble\s+floor\b", decl.group(1))
    assert NAME in hipnlp.EXPORTS
    fn = getattr(hipnlp.load_library(), NAME)     # (AttributeError: the built library does not export it)
    assert fn.argtypes is not None and len(fn.argtypes) == 9


def test_abi_version_is_unchanged():
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (the descriptor did not change)


def test_the_header_no_longer_says_that_no_preconditioner_is_built():
    text = " ".join(open(os.path.join(ROOT, "include", "hipnlp.h")).read().split())
    assert "Building a preconditioner is not part of the library" not in text and "no preconditioner is built here" not in text


@pytest.mark.parametrize("floor", [1e-10, 0.0, -1.0, float("nan"), float("inf")])
def test_a_missing_handle_is_an_invalid_argument(floor):
    lib = hipnlp.load_library()
    assert lib.hipnlp_kkt_diag_precond_device(None, None, None, None, None, floor, None, None, None) == _abi.E_INVALID


def test_binding_and_autograd_surface():
    p = inspect.signature(hipnlp.HipNlp.kkt_diag_precond_device).parameters
    assert list(p) == ["self", "hess_values_ptr", "jac_values_ptr", "minv_top_ptr", "minv_bottom_ptr", "dx_ptr", "dc_ptr", "floor", "stream"]
    assert all(p[k].default == 0 for k in ("dx_ptr", "dc_ptr", "stream")) and p["floor"].default > 0.0
    q = inspect.signature(autograd.KKTValues.diagonal_preconditioner).parameters
    assert list(q) == ["self", "floor"] and q["floor"].default == 1e-10
    doc = " ".join(autograd.KKTValues.diagonal_preconditioner.__doc__.split())
    assert NAME in doc and "nobody has tuned" in doc
    assert NAME in autograd.__doc__
    # solve keeps its signature, its defaults and its disclaimer
    s = inspect.signature(autograd.KKTValues.solve).parameters
    assert list(s) == ["self", "rhs_top", "rhs_bottom", "rtol", "maxiter", "minv", "check_every"]
    assert (s["rtol"].default, s["maxiter"].default, s["minv"].default, s["check_every"].default) == (1e-8, 200, None, 16)
    sdoc = " ".join(autograd.KKTValues.solve.__doc__.split())
    assert "No convergence is promised" in sdoc and "diagonal_preconditioner" in sdoc


class _Engine:
    """stands in for a handle: records the one call a valid build makes"""

    def __init__(self):
        self.calls = []

    def hess_nnz(self):
        return 7

    nnz = 5

    def kkt_diag_precond_device(self, *args, **kw):
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


def test_diagonal_preconditioner_checks_its_arguments_before_any_launch():
    import torch
    nlp = _Nlp()
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    K = autograd.KKTValues(nlp, z(2, 7), z(2, 5), z(2, 4), z(2, 3))
    for bad in (0.0, -1e-10, float("nan"), float("inf"), "1e-10", None, True):
        with pytest.raises(ValueError):
            K.diagonal_preconditioner(floor=bad)
    assert nlp.engine.calls == []                                            # nothing reached the engine
    top, bottom = K.diagonal_preconditioner()
    assert len(nlp.engine.calls) == 1
    args, kw = nlp.engine.calls[0]
    assert args == (K.hess.data_ptr(), K.jac.data_ptr(), top.data_ptr(), bottom.data_ptr())
    assert kw == dict(dx_ptr=K.dx.data_ptr(), dc_ptr=K.dc.data_ptr(), floor=1e-10, stream=0)
    assert top.shape == (2, 4) and bottom.shape == (2, 3) and top.dtype == bottom.dtype == torch.float64 and top.is_contiguous() and bottom.is_contiguous()
    # the operator's own diagonals: with_diagonals gives the matching preconditioner
    dx2 = z(2, 4)
    K.with_diagonals(dx2, None).diagonal_preconditioner(floor=0.5)
    assert len(nlp.engine.calls) == 2
    assert nlp.engine.calls[1][1] == dict(dx_ptr=dx2.data_ptr(), dc_ptr=0, floor=0.5, stream=0)
    K.with_diagonals(None, None).diagonal_preconditioner()
    assert nlp.engine.calls[2][1]["dx_ptr"] == 0 and nlp.engine.calls[2][1]["dc_ptr"] == 0
