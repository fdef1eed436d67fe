"""The C-ABI, the ctypes binding and the torch entry point of the condensed block factorisation (hipnlp_kkt_condensed_factor_device;
HipNlp.kkt_condensed_factor_device; hippopt_amd.autograd.KKTValues.condensed_preconditioner): declaration, export, every refusal of
knot_condense.h's kc_factor_call_error — the one text the library calls before it touches a device, here through the emulation —
condensed_preconditioner's checks in front of any launch, what its docstring and the header state about the inertia, and that
block_preconditioner's object is what it was.  CPU only."""
import inspect
import os
import re
import types

import pytest

import kkt_condensed_emu_lib as kc
from hippopt_amd import _abi, autograd, hipnlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hipnlp_kkt_condensed_factor_device"


def test_entry_point_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipnlp.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(\s*hipnlp_handle\s*\*([^;]*)\)\s*;" % NAME, src)
    assert decl, "not declared in include/hipnlp.h"
    args = [a.strip() for a in decl.group(1).split(",")][1:]
    kinds = ["d" if re.fullmatch(r"double\s+\w+", a) else "p" if "*" in a else "?" for a in args]
    assert "".join(kinds) == "pppp" + "d" + "p" * 9                              # hess, jac, dx, dc; floor; six arrays, two diagonals, stream
    assert NAME in hipnlp.EXPORTS
    fn = getattr(hipnlp.load_library(), NAME)     # (AttributeError: the built library does not export it)
    import ctypes as C
    assert fn.argtypes is not None and len(fn.argtypes) == 15
    assert ["d" if t is C.c_double else "p" for t in fn.argtypes[1:]] == kinds    # the binding's types are the declaration's
    assert callable(hipnlp.HipNlp.kkt_condensed_factor_device)
    assert _abi.ABI_VERSION == 3 == hipnlp.load_library().hipnlp_abi_version()   # (an added symbol; no structure of include/hipnlp.h changed)


def test_a_missing_handle_is_an_invalid_argument():
    lib = hipnlp.load_library()
    assert lib.hipnlp_kkt_condensed_factor_device(*([None] * 5 + [1e-10] + [None] * 9)) == _abi.E_INVALID


def test_the_library_refuses_by_the_text_the_emulation_states_and_launches_once():
    src = open(os.path.join(ROOT, "hippopt_amd", "csrc", "hipnlp.hip")).read()
    body = src[src.index("int %s(" % NAME):]
    body = body[:body.index("\n}\n")]
    assert src.count("kc_factor_call_error(") == 1 and body.count("kc_factor_call_error(") == 1
    assert body.index("kc_factor_call_error(") < body.index("_prepare(") < body.index("kc_build_tables(") < body.index("hipLaunchKernelGGL(")
    assert body.count("hipLaunchKernelGGL(") == 1 and "hipnlp_kkt_condensed_factor_kernel" in body   # ONE launch
    assert "HIPNLP_E_UNSUPPORTED" in body[body.index("kc_build_tables("):body.index("upload_table(")]  # a layout beyond the staging is refused, not truncated


def test_every_refusal_without_a_device():
    ok = dict(hess=1, jac=1, dc=1, floor=1e-10, factor=1, pivots=1, e=1, o=1, inertia=1, status=1, minv_top=1, minv_bottom=1)
    err = lambda **kw: kc.factor_call_error(*dict(ok, **kw).values())  # noqa: E731
    assert err() is None
    for k in ("hess", "jac", "dc", "factor", "pivots", "e", "o", "inertia", "status", "minv_top", "minv_bottom"):
        assert err(**{k: 0}), k
    assert "dc_dev is required" in err(dc=0)
    for floor in (0.0, -1e-10, float("nan"), float("inf")):
        assert "floor" in err(floor=floor)
    # the factor entry point's refusals, in its words
    import kkt_block_emu_lib as kb
    fac = kb.call_errors()["factor"]
    assert err(hess=0) == fac(0, 1e-10, 1, 1, 1, 1, 1, 1)
    assert err(floor=0.0, minv_top=0) == fac(1, 0.0, 1, 1, 1, 1, 1, 1)
    assert err(status=0) == fac(1, 1e-10, 1, 1, 1, 1, 1, 0)


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


def values(dc):
    nlp = types.SimpleNamespace(batch=2, n=384, m=100, device="dev", engine=Recorder())
    nlp._on_current_stream = lambda launch: launch(77)
    K = autograd.KKTValues.__new__(autograd.KKTValues)
    K.nlp, K.hess, K.jac, K.dx, K.dc = nlp, FakeTensor("hess"), FakeTensor("jac"), None, dc
    return nlp, K


def test_condensed_preconditioner_raises_without_dc_and_checks_the_floor_before_any_launch(monkeypatch):
    monkeypatch.setattr(autograd, "_torch", lambda: types.SimpleNamespace())
    nlp, K = values(None)
    with pytest.raises(ValueError, match="dc"):
        K.condensed_preconditioner()
    assert nlp.engine.calls == []
    nlp, K = values(FakeTensor("dc"))
    for floor in (0.0, -1.0, float("inf"), float("nan"), True, "1e-10"):
        with pytest.raises(ValueError, match="floor"):
            K.condensed_preconditioner(floor=floor)
    assert nlp.engine.calls == []


def test_condensed_preconditioner_defaults_and_what_the_docs_state_about_the_inertia():
    sig = inspect.signature(autograd.KKTValues.condensed_preconditioner)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("floor", 1e-10)]
    doc = autograd.KKTValues.condensed_preconditioner.__doc__
    for words in ("raises ValueError without dc", "principal submatrix of C", "does NOT", "(n, m, 0)", "proves NOTHING", "off-diagonal blocks", "NOT claimed",
                  "profiles/r18_kkt_condensed.txt", "hipnlp_kkt_condensed_factor_device", "Haynsworth"):
        assert words in doc, words
    header = open(os.path.join(ROOT, "include", "hipnlp.h")).read()
    at = header.index("The CONDENSED block factorisation")
    comment = header[at:header.index("int %s(" % NAME, at)]
    for words in ("principal submatrix of C", "does NOT", "(n, m, 0)", "proves nothing", "off-diagonal blocks", "ascending global row", "no atomics", "1 620", "439",
                  "a null dc_dev"):
        assert words in comment, words
    for path in ("README.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().lower().split())       # (a paragraph breaks its lines anywhere)
        at = text.index("condensed_preconditioner")
        for words in ("principal submatrix", "not claimed", "off-diagonal blocks", "r18_kkt_condensed.txt"):
            assert words in text[at:], (path, words)


def test_the_block_preconditioners_object_carries_the_flag_and_keeps_its_constructor():
    parts = [FakeTensor(s) for s in ("factor", "pivots", "e", "o", "inertia", "status", "top", "bottom")]
    pre = autograd.KKTBlockPreconditioner(types.SimpleNamespace(nlp=object()), *parts)
    assert pre.condensed is False and (pre.delta, pre.tries, pre.quasi_definite) == (None, None, None)
    params = list(inspect.signature(autograd.KKTBlockPreconditioner.__init__).parameters.values())
    assert [p.name for p in params if p.kind == p.POSITIONAL_OR_KEYWORD] == ["self", "values", "factor", "pivots", "e", "o", "inertia", "status", "top_diagonal", "bottom"]
