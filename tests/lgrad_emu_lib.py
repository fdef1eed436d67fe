"""ctypes access to the TEST-ONLY CPU emulation of the Lagrangian-gradient kernel (tests/lgrad_emu)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hippopt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libhipnlp_lgrad_emu.so")
SRC = [os.path.join(ROOT, "tests", "lgrad_emu", "lgrad_emu.cpp")] + [
    os.path.join(ROOT, "hippopt_amd", "csrc", f) for f in ("layout.h", "knot_body.h", "knot_lgrad.h", "nlp_defs.h", "knot_tanh.h")] + [
    os.path.join(ROOT, "include", "hipnlp.h")]


def build():
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", SO + ".tmp", SRC[0]])
        os.replace(SO + ".tmp", SO)
    return SO


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class LgradEmu:
    def __init__(self, settings, model, detect_simple_bounds=False, jac_varying_first=False):
        self.lib = C.CDLL(build())
        self.lib.lgemu_create.restype = C.c_void_p
        self.desc = _abi.DescC()
        self.desc.settings = settings.to_c()
        self.desc.model = model.to_c()
        self.desc.batch = 1
        self.desc.knot_begin, self.desc.knot_end = 0, settings.horizon_length
        self.desc.flags = (_abi.FLAG_DETECT_SIMPLE_BOUNDS if detect_simple_bounds else 0) | (_abi.FLAG_JAC_VARYING_FIRST if jac_varying_first else 0)
        err = C.create_string_buffer(256)
        self.h = self.lib.lgemu_create(C.byref(self.desc), err, 256)
        if not self.h:
            raise RuntimeError(err.value.decode())
        n, m, nnz = C.c_int(), C.c_int(), C.c_int()
        self.lib.lgemu_dims(C.c_void_p(self.h), C.byref(n), C.byref(m), C.byref(nnz))
        self.n, self.m, self.nnz = n.value, m.value, nnz.value

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.lgemu_destroy(C.c_void_p(self.h))
            self.h = None

    def sparsity(self):
        ir, jc = np.zeros(self.nnz, np.int32), np.zeros(self.nnz, np.int32)
        self.lib.lgemu_sparsity(C.c_void_p(self.h), ir.ctypes.data_as(C.POINTER(C.c_int)), jc.ctypes.data_as(C.POINTER(C.c_int)))
        return ir, jc

    def kept_rows(self):
        """row of this layout behind every row of the full subject_to list (-1: lifted into a bound)"""
        out = np.zeros(self.lib.lgemu_m_full(C.c_void_p(self.h)), np.int32)
        self.lib.lgemu_lift_map(C.c_void_p(self.h), out.ctypes.data_as(C.POINTER(C.c_int)))
        return out

    def tables_ok(self):
        err = C.create_string_buffer(256)
        ok = self.lib.lgemu_tables_ok(C.c_void_p(self.h), err, 256)
        return bool(ok), err.value.decode()

    def table_sizes(self):
        """(entries of a first / interior / last block, multiplier rows of each, entries of the horizon-global columns)"""
        e, r, g = (C.c_int * 3)(), (C.c_int * 3)(), C.c_int()
        self.lib.lgemu_table_sizes(C.c_void_p(self.h), e, r, C.byref(g))
        return list(e), list(r), g.value

    def lagrangian_grad(self, x, p, sigma, lam, out=None):
        """(out [n], writes [n]): sigma grad f + J^T lam, and how often every entry of out was stored"""
        out = np.full(self.n, np.nan) if out is None else out
        writes = np.zeros(self.n, np.int32)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        assert lam.shape == (self.m,)
        rc = self.lib.lgemu_lagrangian_grad(C.c_void_p(self.h), _dp(np.ascontiguousarray(x, dtype=np.float64)), _dp(np.ascontiguousarray(p, dtype=np.float64)),
                                            C.c_double(float(sigma)), _dp(lam), _dp(out), writes.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise RuntimeError("lgemu_lagrangian_grad: %s" % ("tables do not fit the kernel" if rc < 0 else "%d multiplier rows outside [0, m)" % rc))
        return out, writes
