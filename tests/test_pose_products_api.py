"""The C-ABI and the torch entry point of the pose finder's products (hipnlp_pose_eval_lagrangian_grad_device,
hipnlp_pose_eval_jac_vec_device, hipnlp_pose_eval_hess_vec_device; hippopt_amd.autograd.PoseNLP).  CPU only."""
import os
import re

import pytest

from hippopt_amd import _abi, hipnlp
from hippopt_amd.pose_settings import pose_finder_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hipnlp_pose_eval_lagrangian_grad_device", "hipnlp_pose_eval_jac_vec_device", "hipnlp_pose_eval_hess_vec_device")


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_exported_and_bound(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*hipnlp_pose_handle\s*\*" % name, src), "not declared in include/hipnlp.h"
    assert name in hipnlp.EXPORTS
    lib = hipnlp.load_library()
    fn = getattr(lib, name)          # (AttributeError: the built library does not export it)
    assert fn.argtypes is not None and len(fn.argtypes) == (7 if name.endswith("hess_vec_device") else 6)


def test_abi_version_is_unchanged():
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (no structure of include/hipnlp.h changed)


def test_binding_has_the_three_methods():
    for meth in ("eval_lagrangian_grad_device", "eval_jac_vec_device", "eval_hess_vec_device"):
        assert callable(getattr(hipnlp.HipPose, meth))


def test_pose_nlp_without_a_device_fails_loudly(model):
    """no CPU fallback: without a HIP device the handle is refused with E_NODEVICE"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from hippopt_amd.autograd import PoseNLP
    with pytest.raises(hipnlp.HipNlpError) as err:
        PoseNLP(pose_finder_settings(model), model, batch=2)
    assert err.value.code == _abi.E_NODEVICE
    assert "no CPU fallback" in str(err.value)
