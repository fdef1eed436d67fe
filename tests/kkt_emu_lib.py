"""ctypes access to the TEST-ONLY CPU emulation of the one-launch KKT operator (tests/kkt_emu)."""
import ctypes as C

import numpy as np

import emu_build
from emu_build import ROOT, dp as _dp, ip as _ip  # noqa: F401  (re-exported)
from hippopt_amd import _abi

SO = emu_build.library("kkt_emu")
SRC = emu_build.sources("kkt_emu")
NXK = 189


def build():
    return emu_build.build(SO, SRC)


class KktEmu:
    def __init__(self, settings, model, detect_simple_bounds=False, jac_varying_first=False):
        self.lib = C.CDLL(build())
        self.lib.kktemu_create.restype = C.c_void_p
        self.desc = _abi.DescC()
        self.desc.settings = settings.to_c()
        self.desc.model = model.to_c()
        self.desc.batch = 1
        self.desc.knot_begin, self.desc.knot_end = 0, settings.horizon_length
        self.desc.flags = (_abi.FLAG_DETECT_SIMPLE_BOUNDS if detect_simple_bounds else 0) | (_abi.FLAG_JAC_VARYING_FIRST if jac_varying_first else 0)
        err = C.create_string_buffer(256)
        self.h = self.lib.kktemu_create(C.byref(self.desc), err, 256)
        if not self.h:
            raise RuntimeError(err.value.decode())
        n, m, nnz, nnz_h = C.c_int(), C.c_int(), C.c_int(), C.c_long()
        self.lib.kktemu_dims(C.c_void_p(self.h), C.byref(n), C.byref(m), C.byref(nnz), C.byref(nnz_h))
        self.n, self.m, self.nnz, self.nnz_h = n.value, m.value, nnz.value, nnz_h.value
        self.N = settings.horizon_length

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.kktemu_destroy(C.c_void_p(self.h))
            self.h = None

    def sparsity(self):
        ir, jc = np.zeros(self.nnz, np.int32), np.zeros(self.nnz, np.int32)
        self.lib.kktemu_sparsity(C.c_void_p(self.h), _ip(ir), _ip(jc))
        return ir, jc

    def hess_sparsity(self):
        ir, jc = np.zeros(self.nnz_h, np.int32), np.zeros(self.nnz_h, np.int32)
        self.lib.kktemu_hess_sparsity(C.c_void_p(self.h), _ip(ir), _ip(jc))
        return ir, jc

    def kkt_times(self, hess, jac, v, w, dx=None, dc=None):
        """(top [n], bottom [m], top_writes [n], bottom_writes [m]): (H + diag dx) v + J^T w and J v - diag(dc) w from the value runs hess
        [nnz_h] and jac [nnz], the device kernel's way; the destinations start as NaN"""
        cont = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        hess, jac, v, w, dx, dc = cont(hess), cont(jac), cont(v), cont(w), cont(dx), cont(dc)
        assert hess.shape == (self.nnz_h,) and jac.shape == (self.nnz,) and v.shape == (self.n,) and w.shape == (self.m,)
        assert (dx is None or dx.shape == (self.n,)) and (dc is None or dc.shape == (self.m,))
        top, bottom = np.full(self.n, np.nan), np.full(self.m, np.nan)
        tw, bw = np.zeros(self.n, np.int32), np.zeros(self.m, np.int32)
        self.lib.kktemu_times(C.c_void_p(self.h), _dp(hess), _dp(jac), _dp(dx), _dp(dc), _dp(v), _dp(w), _dp(top), _dp(bottom), _ip(tw), _ip(bw))
        return top, bottom, tw, bw
