"""ctypes access to the TEST-ONLY CPU emulation of the stored-values Jacobian products (tests/jprod_emu)."""
import ctypes as C

import numpy as np

import emu_build
from emu_build import dp as _dp, ip as _ip, lp as _lp
from hippopt_amd import _abi

SO = emu_build.library("jprod_emu")
SRC = emu_build.sources("jprod_emu")
NXK = 189


def build():
    return emu_build.build(SO, SRC)


class JprodEmu:
    def __init__(self, settings, model, detect_simple_bounds=False, jac_varying_first=False):
        self.lib = C.CDLL(build())
        self.lib.jpemu_create.restype = C.c_void_p
        self.lib.jpemu_row_directory.restype = C.c_long
        self.lib.jpemu_col_directory.restype = C.c_long
        self.desc = _abi.DescC()
        self.desc.settings = settings.to_c()
        self.desc.model = model.to_c()
        self.desc.batch = 1
        self.desc.knot_begin, self.desc.knot_end = 0, settings.horizon_length
        self.desc.flags = (_abi.FLAG_DETECT_SIMPLE_BOUNDS if detect_simple_bounds else 0) | (_abi.FLAG_JAC_VARYING_FIRST if jac_varying_first else 0)
        err = C.create_string_buffer(256)
        self.h = self.lib.jpemu_create(C.byref(self.desc), err, 256)
        if not self.h:
            raise RuntimeError(err.value.decode())
        n, m, nnz = C.c_int(), C.c_int(), C.c_int()
        self.lib.jpemu_dims(C.c_void_p(self.h), C.byref(n), C.byref(m), C.byref(nnz))
        self.n, self.m, self.nnz = n.value, m.value, nnz.value
        self.N = settings.horizon_length

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.jpemu_destroy(C.c_void_p(self.h))
            self.h = None

    def sparsity(self):
        ir, jc = np.zeros(self.nnz, np.int32), np.zeros(self.nnz, np.int32)
        self.lib.jpemu_sparsity(C.c_void_p(self.h), _ip(ir), _ip(jc))
        return ir, jc

    def counts(self):
        """dict: per pair variant (first, second, interior, last knot) the owned rows and their entries; the entries of the first block
        the last knot stages; the horizon-global entries; per block variant the entries and the multipliers"""
        out = np.zeros(16, np.int32)
        self.lib.jpemu_counts(C.c_void_p(self.h), _ip(out))
        return {"rows": out[0:4].tolist(), "entries": out[4:8].tolist(), "other": int(out[8]), "glob": int(out[9]),
                "block": out[10:13].tolist(), "multipliers": out[13:16].tolist()}

    def row_directory(self):
        """(owners [m], idx, row, knot, var): how many knots own every row; the entries of the row directory over the horizon in the
        order of the sums, as the device's table words say: pattern index, row, owner knot, variable of v"""
        cap = self.nnz + 16
        owners = np.zeros(self.m, np.int32)
        idx, row, knot, var = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int64)
        t = self.lib.jpemu_row_directory(C.c_void_p(self.h), _ip(owners), C.c_long(cap), _lp(idx), _ip(row), _ip(knot), _lp(var))
        assert t >= 0, "more directory entries than pattern entries"
        return owners, idx[:t], row[:t], knot[:t], var[:t]

    def col_directory(self):
        """(idx, col, row): the entries of the column directory over the horizon in the order of the sums"""
        cap = self.nnz + 16
        idx, col, row = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        t = self.lib.jpemu_col_directory(C.c_void_p(self.h), C.c_long(cap), _lp(idx), _ip(col), _ip(row))
        assert t >= 0, "more directory entries than pattern entries"
        return idx[:t], col[:t], row[:t]

    def jac_times(self, values, v, grad=None, want_jv=True, want_dot=None):
        """(jv [m] or None, dot or None, jv_writes [m], dot_writes): J v and grad . v from a value run, the device kernels' way"""
        want_dot = grad is not None if want_dot is None else want_dot
        values = np.ascontiguousarray(values, dtype=np.float64)
        v = np.ascontiguousarray(v, dtype=np.float64)
        grad = None if grad is None else np.ascontiguousarray(grad, dtype=np.float64)
        assert values.shape == (self.nnz,) and v.shape == (self.n,) and (grad is None or grad.shape == (self.n,))
        jv = np.full(self.m, np.nan) if want_jv else None
        dot = np.full(1, np.nan) if want_dot else None
        jw, dw = np.zeros(self.m, np.int32), np.zeros(1, np.int32)
        self.lib.jpemu_jac_times(C.c_void_p(self.h), _dp(values), _dp(grad), _dp(v), _dp(jv), _dp(dot), _ip(jw), _ip(dw))
        return jv, (float(dot[0]) if want_dot else None), jw, int(dw[0])

    def jac_transpose_times(self, values, lam, sigma=0.0, grad=None):
        """(out [n], writes [n]): sigma grad + J^T lam (grad None: J^T lam) from a value run, the device kernel's way"""
        values = np.ascontiguousarray(values, dtype=np.float64)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        grad = None if grad is None else np.ascontiguousarray(grad, dtype=np.float64)
        assert values.shape == (self.nnz,) and lam.shape == (self.m,) and (grad is None or grad.shape == (self.n,))
        out, writes = np.full(self.n, np.nan), np.zeros(self.n, np.int32)
        self.lib.jpemu_jac_transpose_times(C.c_void_p(self.h), _dp(values), _dp(grad), C.c_double(float(sigma)), _dp(lam), _dp(out), _ip(writes))
        return out, writes
