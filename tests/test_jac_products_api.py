"""The C-ABI, the ctypes binding and the torch entry points of the products with a stored value run of jac g
(hipnlp_jac_times_device, hipnlp_jac_transpose_times_device; HipNlp.jac_times_device / jac_transpose_times_device;
hippopt_amd.autograd.JacobianValues).  CPU only."""
import inspect
import os
import re

import pytest

from hippopt_amd import _abi, autograd, hipnlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hipnlp_jac_times_device", "hipnlp_jac_transpose_times_device")


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_exported_and_bound(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(\s*hipnlp_handle\s*\*([^;]*)\)\s*;" % name, src)
    assert decl, "not declared in include/hipnlp.h"
    assert decl.group(1).count(",") == 6          # handle + five pointers + stream
    assert name in hipnlp.EXPORTS
    fn = getattr(hipnlp.load_library(), name)     # (AttributeError: the built library does not export it)
    assert fn.argtypes is not None and len(fn.argtypes) == 7


def test_abi_version_is_unchanged():
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (no structure of include/hipnlp.h changed)


def test_a_missing_handle_is_an_invalid_argument():
    """the one error code that needs no device: HIPNLP_E_INVALID before anything is dereferenced"""
    lib = hipnlp.load_library()
    assert lib.hipnlp_jac_times_device(None, None, None, None, None, None, None) == _abi.E_INVALID
    assert lib.hipnlp_jac_transpose_times_device(None, None, None, None, None, None, None) == _abi.E_INVALID


def test_binding_and_autograd_surface():
    for meth in ("jac_times_device", "jac_transpose_times_device"):
        assert callable(getattr(hipnlp.HipNlp, meth))
    for meth in ("matvec", "grad_dot", "jvp", "rmatvec"):
        assert callable(getattr(autograd.JacobianValues, meth))
    assert callable(autograd.KinodynamicNLP.jacobian)
    sig = inspect.signature(autograd.KinodynamicNLP.__init__)
    assert sig.parameters["jacobian_products"].default is False          # opt-in: the default still raises
    assert list(inspect.signature(autograd.KinodynamicNLP.jacobian_vector_product).parameters) == \
        list(inspect.signature(autograd.PoseNLP.jacobian_vector_product).parameters)
    assert "two launches" in autograd.KinodynamicNLP.jacobian_vector_product.__doc__.lower()


def test_layouts_of_the_planners_are_inside_the_caps(model):
    """the capacities the device kernels stage are checked by the layout build (jprod_ok / jprod_error; a layout beyond them is
    refused): the planners' layouts are inside them, with the margins DESIGN.md states"""
    from jprod_emu_lib import JprodEmu
    from hippopt_amd.kinodyn_settings import periodic_step_settings, stairs_settings
    for mk in (periodic_step_settings, stairs_settings):
        c = JprodEmu(mk(5, model), model).counts()
        assert max(c["rows"]) <= 512 and max(c["entries"]) <= 2048 and max(c["block"]) <= 1792 and c["other"] <= 128 and c["glob"] <= 16
