"""The C-ABI, the ctypes binding and the torch entry point of the per-knot inertia-correcting ladder (hipnlp_kkt_block_ladder_device;
HipNlp.kkt_block_ladder_device; hippopt_amd.autograd.KKTValues.convexify): declaration, export, every refusal of knot_ldl.h's
kl_ladder_call_error — the one text the library calls before it touches a device, here through the emulation — convexify's checks in
front of any launch, and that block_preconditioner is what it was.  CPU only."""
import inspect
import os
import re
import types

import pytest

import kkt_ladder_emu_lib as kl
from hippopt_amd import _abi, autograd, hipnlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hipnlp_kkt_block_ladder_device"


def test_entry_point_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(\s*hipnlp_handle\s*\*([^;]*)\)\s*;" % NAME, src)
    assert decl, "not declared in include/hipnlp.h"
    assert decl.group(1).count(",") == 16 - 1
    assert NAME in hipnlp.EXPORTS
    fn = getattr(hipnlp.load_library(), NAME)     # (AttributeError: the built library does not export it)
    assert fn.argtypes is not None and len(fn.argtypes) == 16
    assert callable(hipnlp.HipNlp.kkt_block_ladder_device)


def test_abi_version_is_unchanged():
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (no structure of include/hipnlp.h changed)


def test_a_missing_handle_is_an_invalid_argument():
    lib = hipnlp.load_library()
    assert lib.hipnlp_kkt_block_ladder_device(*([None] * 3 + [1e-10, 1e-4, 8.0, 16] + [None] * 9)) == _abi.E_INVALID


def test_the_library_refuses_by_the_text_the_emulation_states():
    src = open(os.path.join(ROOT, "hippopt_amd", "csrc", "hipnlp.hip")).read()
    body = src[src.index("int %s(" % NAME):]
    body = body[:body.index("\n}\n")]
    assert src.count("kl_ladder_call_error(") == 1 and body.count("kl_ladder_call_error(") == 1
    assert body.index("kl_ladder_call_error(") < body.index("_prepare(") < body.index("hipLaunchKernelGGL(")
    assert body.count("hipLaunchKernelGGL(") == 1 and "hipnlp_kkt_block_ladder_kernel" in body       # ONE launch


def test_every_refusal_without_a_device():
    ok = dict(hess=1, floor=1e-10, delta_init=1e-4, kappa=8.0, max_tries=16, factor=1, pivots=1, e=1, o=1, inertia=1, status=1, delta=1, tries=1)
    err = lambda **kw: kl.ladder_call_error(*dict(ok, **kw).values())  # noqa: E731
    assert err() is None
    for k in ("hess", "factor", "pivots", "e", "o", "inertia", "status", "delta", "tries"):
        assert err(**{k: 0}), k
    for floor in (0.0, -1e-10, float("nan"), float("inf")):
        assert "floor" in err(floor=floor)
    for mt in (-1, 17, 1000):
        assert "max_tries" in err(max_tries=mt)
    assert err(max_tries=0) is None and err(max_tries=1) is None
    for bad in (0.0, -1e-4, float("nan"), float("inf")):
        assert "delta_init" in err(delta_init=bad)
        assert err(delta_init=bad, max_tries=0) is None                          # (not read without a ladder)
    for bad in (1.0, 0.5, -8.0, float("nan"), float("inf")):
        assert "kappa" in err(kappa=bad)
        assert err(kappa=bad, max_tries=0) is None
    # the factor entry point's refusals come first, in its words
    import kkt_block_emu_lib as kb
    fac = kb.call_errors()["factor"]
    assert err(hess=0, max_tries=99) == fac(0, 1e-10, 1, 1, 1, 1, 1, 1)
    assert err(floor=0.0, kappa=0.0) == fac(1, 0.0, 1, 1, 1, 1, 1, 1)
    c = kl.caps()
    assert (c["max_tries"], c["ok"], c["nonfinite"], c["exhausted"]) == (16, 0, 2, 3)


class FakeTensor:
    def __init__(self, name):
        self.name = name
        self.device = "dev"

    def data_ptr(self):
        return 1000 + sum(map(ord, self.name))


class Recorder:
    """stands where HipNlp stands in a KinodynamicNLP: records every call that would reach the device"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("kkt_"):
            return lambda *a, **kw: self.calls.append((name, a, kw))
        raise AttributeError(name)


def test_convexify_checks_its_arguments_before_any_launch(monkeypatch):
    nlp = types.SimpleNamespace(batch=2, n=384, m=100, device="dev", engine=Recorder())
    nlp._on_current_stream = lambda launch: launch(77)
    touched = []
    monkeypatch.setattr(autograd, "_torch", lambda: touched.append("torch") or types.SimpleNamespace())
    K = autograd.KKTValues.__new__(autograd.KKTValues)
    K.nlp, K.hess, K.jac, K.dx, K.dc = nlp, FakeTensor("hess"), FakeTensor("jac"), None, None
    bad = [dict(floor=f) for f in (0.0, -1.0, float("inf"), float("nan"), True, "1e-10")]
    bad += [dict(max_tries=t) for t in (-1, 17, 2.0, True, "3", None)]
    bad += [dict(delta_init=v) for v in (0.0, -1e-4, float("inf"), float("nan"), True, "1e-4", None)]
    bad += [dict(kappa=v) for v in (1.0, 0.5, -8.0, float("inf"), float("nan"), True, "8", None)]
    for kw in bad:
        with pytest.raises(ValueError):
            K.convexify(**kw)
    assert nlp.engine.calls == []


def test_convexify_defaults_and_what_its_docstring_states():
    sig = inspect.signature(autograd.KKTValues.convexify)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("delta_init", 1e-4), ("kappa", 8.0), ("max_tries", 16), ("floor", 1e-10)]
    doc = autograd.KKTValues.convexify.__doc__
    for words in ("(n, m, 0)", "NOT guaranteed", "minimal in IPOPT's sense", "MINRES converges", "first_hessian_perturbation", "perturb_inc_fact", "nobody has tuned",
                  "profiles/r17_kkt_ladder.txt", "hipnlp_kkt_block_ladder_device"):
        assert words in doc, words
    header = open(os.path.join(ROOT, "include", "hipnlp.h")).read()
    at = header.index("The inertia-correcting ladder")
    comment = header[at:header.index("int %s(" % NAME, at)]
    for words in ("quasi-definite", "(n, m, 0)", "SUFFICIENT", "NOT IPOPT's criterion", "no status 1", "3 the ladder was exhausted", "max_tries = 0"):
        assert words in comment, words


def test_block_preconditioner_and_its_object_are_what_they_were():
    sig = inspect.signature(autograd.KKTValues.block_preconditioner)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [("self", inspect.Parameter.empty), ("floor", 1e-10)]
    doc = autograd.KKTValues.block_preconditioner.__doc__
    assert doc.startswith("KKTBlockPreconditioner: M^-1 = blockdiag_k(P_k^T L_k^-T |D_k|^-1 L_k^-1 P_k)") and doc.rstrip().endswith("converge.")
    for words in ("nothing is\n        retried or regularised", "NOT claimed", "1e-4 smaller", "2 425", "515", "profiles/r16_kkt_block.txt"):
        assert words in doc, words
    assert "ladder" not in doc and "convexify" not in doc
    params = list(inspect.signature(autograd.KKTBlockPreconditioner.__init__).parameters.values())
    positional = [p.name for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert positional == ["self", "values", "factor", "pivots", "e", "o", "inertia", "status", "top_diagonal", "bottom"]
    assert [(p.name, p.default) for p in params if p.kind == p.KEYWORD_ONLY] == [("delta", None), ("tries", None), ("quasi_definite", None)]
    parts = [FakeTensor(s) for s in ("factor", "pivots", "e", "o", "inertia", "status", "top", "bottom")]
    values = types.SimpleNamespace(nlp=object())
    pre = autograd.KKTBlockPreconditioner(values, *parts)
    assert pre.values is values and (pre.delta, pre.tries, pre.quasi_definite) == (None, None, None)
