"""ctypes access to the TEST-ONLY CPU emulation of the Hessian-vector kernels (tests/hvp_emu)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hippopt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libhipnlp_hvp_emu.so")
SRC = [os.path.join(ROOT, "tests", "hvp_emu", "hvp_emu.cpp")] + [
    os.path.join(ROOT, "hippopt_amd", "csrc", f) for f in ("layout.h", "knot_body.h", "knot_hess_body.h", "knot_hess_layout.h", "knot_hess_terrain.h", "knot_hvp.h",
                                                           "knot_lgrad.h", "nlp_defs.h", "knot_tanh.h")] + [
    os.path.join(ROOT, "include", "hipnlp.h")]
NXK = 189


def build():
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", SO + ".tmp", SRC[0]])
        os.replace(SO + ".tmp", SO)
    return SO


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class HvpEmu:
    def __init__(self, settings, model, detect_simple_bounds=False, jac_varying_first=False):
        self.lib = C.CDLL(build())
        self.lib.hvemu_create.restype = C.c_void_p
        self.desc = _abi.DescC()
        self.desc.settings = settings.to_c()
        self.desc.model = model.to_c()
        self.desc.batch = 1
        self.desc.knot_begin, self.desc.knot_end = 0, settings.horizon_length
        self.desc.flags = (_abi.FLAG_DETECT_SIMPLE_BOUNDS if detect_simple_bounds else 0) | (_abi.FLAG_JAC_VARYING_FIRST if jac_varying_first else 0)
        err = C.create_string_buffer(256)
        self.h = self.lib.hvemu_create(C.byref(self.desc), err, 256)
        if not self.h:
            raise RuntimeError(err.value.decode())
        n, m, nnz_h, nnz_knot, n_couple, touches = C.c_int(), C.c_int(), C.c_long(), C.c_int(), C.c_int(), C.c_int()
        self.lib.hvemu_dims(C.c_void_p(self.h), C.byref(n), C.byref(m), C.byref(nnz_h), C.byref(nnz_knot), C.byref(n_couple), C.byref(touches))
        self.n, self.m, self.nnz_h, self.nnz_knot, self.n_couple, self.touches = n.value, m.value, nnz_h.value, nnz_knot.value, n_couple.value, touches.value
        self.N = settings.horizon_length

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.hvemu_destroy(C.c_void_p(self.h))
            self.h = None

    def hess_sparsity(self):
        ir, jc = np.zeros(self.nnz_h, np.int32), np.zeros(self.nnz_h, np.int32)
        self.lib.hvemu_hess_sparsity(C.c_void_p(self.h), _ip(ir), _ip(jc))
        return ir, jc

    def kept_rows(self):
        """row of this layout behind every row of the full subject_to list (-1: lifted into a bound)"""
        out = np.zeros(self.lib.hvemu_m_full(C.c_void_p(self.h)), np.int32)
        self.lib.hvemu_lift_map(C.c_void_p(self.h), _ip(out))
        return out

    def tables(self):
        """dict: beg [190], K [189], couple [189] (coupling entry of the variable or -1), and per touch pos / slot / other"""
        t = {"beg": np.zeros(NXK + 1, np.int32), "K": np.zeros(NXK, np.int32), "couple": np.zeros(NXK, np.int32),
             "pos": np.zeros(self.touches, np.int32), "slot": np.zeros(self.touches, np.int32), "other": np.zeros(self.touches, np.int32)}
        self.lib.hvemu_tables(C.c_void_p(self.h), _ip(t["beg"]), _ip(t["K"]), _ip(t["couple"]), _ip(t["pos"]), _ip(t["slot"]), _ip(t["other"]))
        return t

    def perm(self):
        p, pc = np.zeros(self.nnz_knot, np.int32), np.zeros(self.n_couple, np.int32)
        self.lib.hvemu_perm(C.c_void_p(self.h), _ip(p), _ip(pc))
        return p, pc

    def touch_counts(self):
        """K_i of every variable of the NLP [n]: touches of its knot-record variable, + 1 where it has a coupling term (both horizon
        ends of a handle with the periodicity as a cost); 0 for the horizon-global variables"""
        t = self.tables()
        out = np.zeros(self.n, np.int64)
        for k in range(self.N):
            out[NXK * k:NXK * (k + 1)] = t["K"]
            if self.n_couple and k in (0, self.N - 1):
                out[NXK * k:NXK * (k + 1)] += t["couple"] >= 0
        return out

    def hess_vec(self, x, p, sigma, lam, v, out=None, want_values=False):
        """(out [n], writes [n][, values [nnz_h]]): H(x, sigma, lam) v the fused kernel's way, and how often every entry of out was stored"""
        out = np.full(self.n, np.nan) if out is None else out
        writes = np.zeros(self.n, np.int32)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert lam.shape == (self.m,) and v.shape == (self.n,)
        values = np.full(self.nnz_h, np.nan) if want_values else None
        self.lib.hvemu_hess_vec(C.c_void_p(self.h), _dp(np.ascontiguousarray(x, dtype=np.float64)), _dp(np.ascontiguousarray(p, dtype=np.float64)),
                                C.c_double(float(sigma)), _dp(lam), _dp(v), _dp(out), _ip(writes), _dp(values) if want_values else None)
        return (out, writes, values) if want_values else (out, writes)

    def hess_times(self, values, v, out=None):
        """(out [n], writes [n]): H v from a value run, the stored-values kernel's way"""
        out = np.full(self.n, np.nan) if out is None else out
        writes = np.zeros(self.n, np.int32)
        values = np.ascontiguousarray(values, dtype=np.float64)
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert values.shape == (self.nnz_h,) and v.shape == (self.n,)
        self.lib.hvemu_hess_times(C.c_void_p(self.h), _dp(values), _dp(v), _dp(out), _ip(writes))
        return out, writes
