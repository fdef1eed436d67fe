"""The C-ABI, the ctypes binding and the torch entry points of the one-launch KKT operator from stored value runs
(hipnlp_kkt_times_device; HipNlp.kkt_times_device; hippopt_amd.autograd.KKTValues, KinodynamicNLP.kkt).  CPU only."""
import inspect
import os
import re

from hippopt_amd import _abi, autograd, hipnlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hipnlp_kkt_times_device"


def test_entry_point_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(\s*hipnlp_handle\s*\*([^;]*)\)\s*;" % NAME, src)
    assert decl, "not declared in include/hipnlp.h"
    assert decl.group(1).count(",") == 9          # handle + eight pointers + stream: 10 parameters
    assert NAME in hipnlp.EXPORTS
    fn = getattr(hipnlp.load_library(), NAME)     # (AttributeError: the built library does not export it)
    assert fn.argtypes is not None and len(fn.argtypes) == 10


def test_abi_version_is_unchanged():
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (no structure of include/hipnlp.h changed)


def test_a_missing_handle_is_an_invalid_argument():
    """the one error code that needs no device: HIPNLP_E_INVALID before anything is dereferenced"""
    assert hipnlp.load_library().hipnlp_kkt_times_device(*([None] * 10)) == _abi.E_INVALID


def test_binding_and_autograd_surface():
    assert callable(hipnlp.HipNlp.kkt_times_device)
    p = inspect.signature(hipnlp.HipNlp.kkt_times_device).parameters
    assert p["dx_ptr"].default == 0 and p["dc_ptr"].default == 0 and p["stream"].default == 0
    for meth in ("matvec", "with_diagonals"):
        assert callable(getattr(autograd.KKTValues, meth))
    assert list(inspect.signature(autograd.KKTValues.__init__).parameters) == ["self", "nlp", "hessian_values", "jacobian_values", "dx", "dc"]
    assert list(inspect.signature(autograd.KKTValues.matvec).parameters) == ["self", "v", "w"]
    assert list(inspect.signature(autograd.KinodynamicNLP.kkt).parameters) == ["self", "x", "sigma", "lam", "dx", "dc"]
    assert inspect.signature(autograd.KinodynamicNLP.kkt).parameters["dx"].default is None
    assert "hipnlp_kkt_times_device" in autograd.__doc__ and "one launch" in autograd.KKTValues.__doc__.lower()
