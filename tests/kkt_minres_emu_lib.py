"""ctypes access to the TEST-ONLY CPU emulation of the device-resident MINRES solve on the KKT operator (tests/kkt_minres_emu)."""
import collections
import ctypes as C

import numpy as np

import emu_build
from emu_build import dp as _dp, ip as _ip
from hippopt_amd import _abi
from kkt_emu_lib import KktEmu

SO = emu_build.library("kkt_minres_emu")
SRC = emu_build.sources("kkt_minres_emu", "kkt_emu")

Solution = collections.namedtuple("Solution", "top bottom iterations residual status top_writes bottom_writes scalar_writes trace trace_vec")


def build():
    return emu_build.build(SO, SRC)


class KktMinresEmu(KktEmu):
    """the solve and the operator's emulation (kkt_times and the patterns, KktEmu's methods) on ONE handle of ONE library: this
    emulation's, which holds the operator's emulation too and creates, uses and destroys the handle itself"""

    def __init__(self, settings, model, detect_simple_bounds=False, jac_varying_first=False):
        self.lib = self.mlib = C.CDLL(build())
        self.lib.kktemu_create.restype = C.c_void_p
        self._destroy = self.lib.kktemu_destroy
        self._destroy.argtypes = [C.c_void_p]
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

    def __del__(self):                     # (on its own names only: at interpreter shutdown a module's globals may be gone before a cached emulation is)
        h, self.h = getattr(self, "h", None), None
        if h:
            self._destroy(h)

    def solve(self, hess, jac, rhs_top, rhs_bottom, dx=None, dc=None, minv=None, rtol=1e-8, maxiter=200, launched=None, trace=False, trace_vec=False):
        """Solution of one trajectory: the start and `launched` (default maxiter) iterations' launches, the device's way; the six outputs
        start as NaN / -99 and every store to them is counted.  trace [launched, 6]: alfa, beta, phibar, status, it, ran;
        trace_vec [launched, 4, n + m]: v, y (as alfa sees it), the new r2, M^-1 r2"""
        cont = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        hess, jac, dx, dc, rhs_top, rhs_bottom = cont(hess), cont(jac), cont(dx), cont(dc), cont(rhs_top), cont(rhs_bottom)
        mt, mb = (None, None) if minv is None else (cont(minv[0]), cont(minv[1]))
        assert hess.shape == (self.nnz_h,) and jac.shape == (self.nnz,) and rhs_top.shape == (self.n,) and rhs_bottom.shape == (self.m,)
        assert (dx is None or dx.shape == (self.n,)) and (dc is None or dc.shape == (self.m,)) and (mt is None or (mt.shape == (self.n,) and mb.shape == (self.m,)))
        launched = maxiter if launched is None else launched
        top, bottom = np.full(self.n, np.nan), np.full(self.m, np.nan)
        tw, bw, sw = np.zeros(self.n, np.int32), np.zeros(self.m, np.int32), np.zeros(3, np.int32)
        it, st, res = C.c_int(-99), C.c_int(-99), C.c_double(float("nan"))
        tr = np.full((launched, 6), np.nan) if trace else None
        tv = np.full((launched, 4, self.n + self.m), np.nan) if trace_vec else None
        self.mlib.kmremu_solve(C.c_void_p(self.h), _dp(hess), _dp(jac), _dp(dx), _dp(dc), _dp(mt), _dp(mb), _dp(rhs_top), _dp(rhs_bottom), _dp(top), _dp(bottom),
                              C.c_double(rtol), C.c_int(maxiter), C.c_int(launched), C.byref(it), C.byref(res), C.byref(st), _ip(tw), _ip(bw), _ip(sw), _dp(tr), _dp(tv))
        return Solution(top, bottom, it.value, res.value, st.value, tw, bw, sw, tr, tv)

