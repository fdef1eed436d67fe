"""The C-ABI, the ctypes binding and the torch entry points of the block preconditioner of the KKT solve (hipnlp_kkt_block_bytes,
hipnlp_kkt_block_factor_device, hipnlp_kkt_block_apply_device, hipnlp_kkt_minres_block_device; HipNlp.kkt_block_* / kkt_minres_block_device;
hippopt_amd.autograd.KKTValues.block_preconditioner and KKTBlockPreconditioner): declarations, exports, every refusal of the three entry
points — knot_ldl.h's kl_*_call_error, the one text the library calls before it touches a device, here through the emulation — and the
routing of KKTValues.solve: a pair or None goes to the old entry point, the object to the new one.  CPU only."""
import os
import re

import pytest

import kkt_block_emu_lib as kb
from hippopt_amd import _abi, autograd, hipnlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMETERS = {"hipnlp_kkt_block_bytes": 2, "hipnlp_kkt_block_factor_device": 11, "hipnlp_kkt_block_apply_device": 12, "hipnlp_kkt_minres_block_device": 22}


@pytest.mark.parametrize("name", sorted(PARAMETERS))
def test_entry_point_is_declared_exported_and_bound(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(\s*(?:const\s+)?hipnlp_handle\s*\*([^;]*)\)\s*;" % name, src)
    assert decl, "not declared in include/hipnlp.h"
    assert decl.group(1).count(",") == PARAMETERS[name] - 1
    assert name in hipnlp.EXPORTS
    fn = getattr(hipnlp.load_library(), name)     # (AttributeError: the built library does not export it)
    assert fn.argtypes is not None and len(fn.argtypes) == PARAMETERS[name]


def test_abi_version_is_unchanged():
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (no structure of include/hipnlp.h changed)


def test_a_missing_handle_is_an_invalid_argument():
    lib = hipnlp.load_library()
    assert lib.hipnlp_kkt_block_bytes(None, None) == _abi.E_INVALID
    assert lib.hipnlp_kkt_block_factor_device(*([None] * 3 + [1e-10] + [None] * 7)) == _abi.E_INVALID
    assert lib.hipnlp_kkt_block_apply_device(*([None] * 12)) == _abi.E_INVALID
    assert lib.hipnlp_kkt_minres_block_device(*([None] * 15 + [1e-8, 10, 0] + [None] * 4)) == _abi.E_INVALID


def test_the_library_refuses_by_the_text_the_emulation_states():
    src = open(os.path.join(ROOT, "hippopt_amd", "csrc", "hipnlp.hip")).read()
    body = src[src.index("int hipnlp_kkt_block_factor_device("):src.index("// how a handle in auto mode")]
    for call, entry in (("kl_factor_call_error(", "int hipnlp_kkt_block_factor_device("), ("kl_apply_call_error(", "int hipnlp_kkt_block_apply_device("),
                        ("kl_minres_call_error(", "int hipnlp_kkt_minres_block_device(")):
        assert body.count(call) == 1
        at = body.index(entry)
        assert at < body.index(call) < body.index("hipLaunchKernelGGL(", at)     # the refusal stands in front of the entry point's first launch
        assert body.index(call) < body.index("_prepare(", at)                    # ... and in front of anything that touches the device


def test_every_refusal_without_a_device():
    ce = kb.call_errors()
    fac = dict(hess=1, floor=1e-10, factor=1, pivots=1, e=1, o=1, inertia=1, status=1)
    assert ce["factor"](*fac.values()) is None
    for k in fac:
        if k != "floor":
            assert ce["factor"](*dict(fac, **{k: 0}).values()), k
    for floor in (0.0, -1e-10, float("nan"), float("inf")):
        assert "floor" in ce["factor"](*dict(fac, floor=floor).values())
    app = dict.fromkeys(("factor", "pivots", "e", "o", "minv_top", "minv_bottom", "r_top", "r_bottom", "z_top", "z_bottom"), 1)
    assert ce["apply"](*app.values()) is None
    for k in app:
        assert ce["apply"](*dict(app, **{k: 0}).values()), k
    mr = dict.fromkeys(("hess", "jac", "factor", "pivots", "e", "o", "minv_top", "minv_bottom", "rhs_top", "rhs_bottom", "sol_top", "sol_bottom", "iterations", "residual",
                        "status"), 1)
    mr.update(rtol=1e-8, max_iterations=10, check_every=0)
    assert ce["minres"](*mr.values()) is None
    assert ce["minres"](*dict(mr, rtol=0.0, max_iterations=0).values()) is None
    for k in list(mr)[:15]:
        assert ce["minres"](*dict(mr, **{k: 0}).values()), k
    assert "rtol" in ce["minres"](*dict(mr, rtol=-1.0).values()) and "rtol" in ce["minres"](*dict(mr, rtol=float("nan")).values())
    assert "max_iterations" in ce["minres"](*dict(mr, max_iterations=-1).values())
    assert "check_every" in ce["minres"](*dict(mr, check_every=-1).values())


class FakeTensor:
    def __init__(self, name):
        self.name = name

    def data_ptr(self):
        return 1000 + sum(map(ord, self.name))


class Recorder:
    """stands where HipNlp stands in a KinodynamicNLP: records which entry point a solve goes to"""

    def __init__(self):
        self.calls = []

    def kkt_minres_device(self, *a, **kw):
        self.calls.append(("hipnlp_kkt_minres_device", a, kw))

    def kkt_minres_block_device(self, *a, **kw):
        self.calls.append(("hipnlp_kkt_minres_block_device", a, kw))


def routed(monkeypatch, minv_of):
    """the entry point and arguments K.solve(minv=minv_of(K, nlp)) reaches, with torch and the shape checks stood in for"""
    import types
    nlp = types.SimpleNamespace(batch=2, n=384, m=100, device="dev", engine=Recorder())
    nlp._check = lambda *a: None
    nlp._on_current_stream = lambda launch: launch(77)
    fake_torch = types.SimpleNamespace(empty_like=lambda t, **kw: FakeTensor("like " + t.name), empty=lambda *a, **kw: FakeTensor("empty"), int32="i32", float64="f64",
                                       contiguous_format=None)
    monkeypatch.setattr(autograd, "_torch", lambda: fake_torch)
    K = autograd.KKTValues.__new__(autograd.KKTValues)
    K.nlp, K.hess, K.jac, K.dx, K.dc = nlp, FakeTensor("hess"), FakeTensor("jac"), FakeTensor("dx"), None
    K.solve(FakeTensor("bt"), FakeTensor("bb"), maxiter=5, minv=minv_of(K, nlp), check_every=0)
    assert len(nlp.engine.calls) == 1
    return nlp.engine.calls[0]


def test_solve_routes_a_pair_and_none_to_the_old_entry_point_and_the_object_to_the_new(monkeypatch):
    name, a, kw = routed(monkeypatch, lambda K, nlp: None)
    assert name == "hipnlp_kkt_minres_device" and kw["minv_top_ptr"] == 0 and kw["minv_bottom_ptr"] == 0
    name, a, kw = routed(monkeypatch, lambda K, nlp: (FakeTensor("mt"), FakeTensor("mb")))
    assert name == "hipnlp_kkt_minres_device" and kw["minv_top_ptr"] == FakeTensor("mt").data_ptr() and kw["minv_bottom_ptr"] == FakeTensor("mb").data_ptr()
    parts = [FakeTensor(s) for s in ("factor", "pivots", "e", "o", "inertia", "status", "top", "bottom")]
    name, a, kw = routed(monkeypatch, lambda K, nlp: autograd.KKTBlockPreconditioner(K, *parts))
    assert name == "hipnlp_kkt_minres_block_device"
    assert list(a[:8]) == [FakeTensor(s).data_ptr() for s in ("hess", "jac", "factor", "pivots", "e", "o", "top", "bottom")]
    assert kw["dx_ptr"] == FakeTensor("dx").data_ptr() and kw["dc_ptr"] == 0 and kw["max_iterations"] == 5 and kw["check_every"] == 0 and kw["stream"] == 77


def test_solve_and_block_preconditioner_check_their_arguments_before_any_launch(monkeypatch):
    import types
    other = types.SimpleNamespace(nlp=object())
    with pytest.raises(ValueError):                                              # a preconditioner of another nlp
        routed(monkeypatch, lambda K, nlp: autograd.KKTBlockPreconditioner(other, *[FakeTensor("x")] * 8))
    with pytest.raises(TypeError):
        routed(monkeypatch, lambda K, nlp: "diagonal")
    nlp = types.SimpleNamespace(batch=2, n=384, m=100, device="dev", engine=Recorder())
    K = autograd.KKTValues.__new__(autograd.KKTValues)
    K.nlp, K.hess, K.jac, K.dx, K.dc = nlp, FakeTensor("hess"), FakeTensor("jac"), None, None
    for floor in (0.0, -1.0, float("inf"), float("nan"), True, "1e-10"):
        with pytest.raises(ValueError):
            K.block_preconditioner(floor)
    assert nlp.engine.calls == []


def test_binding_and_autograd_surface():
    for name in ("kkt_block_bytes", "kkt_block_factor_device", "kkt_block_apply_device", "kkt_minres_block_device"):
        assert callable(getattr(hipnlp.HipNlp, name)), name
    assert callable(autograd.KKTValues.block_preconditioner) and callable(autograd.KKTBlockPreconditioner.apply)
    doc = autograd.KKTValues.block_preconditioner.__doc__
    for words in ("NOT claimed", "1e-4 smaller", "2 425", "515", "profiles/r16_kkt_block.txt"):
        assert words in doc, words
    c = kb.caps()
    assert (c["order"], c["doubles"]) == (189, 17955) and c["doubles"] * 8 == 143640
