"""ctypes access to the TEST-ONLY CPU emulation of the pose finder's KKT kernels (tests/pose_kkt_emu): the operator, the diagonal
preconditioner and the whole MINRES solve of one pose, from stored value runs."""
import collections
import ctypes as C

import numpy as np

import emu_build
from emu_build import dp as _dp, ip as _ip
from hippopt_amd import _abi

SO = emu_build.library("pose_kkt_emu")
SRC = emu_build.sources("pose_kkt_emu")

Product = collections.namedtuple("Product", "top bottom top_writes bottom_writes")
Solution = collections.namedtuple("Solution", "top bottom iterations residual status top_writes bottom_writes scalar_writes trace")


def build():
    return emu_build.build(SO, SRC)


def _d(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


class PoseKktEmu:
    def __init__(self, settings, model):
        self.lib = C.CDLL(build())
        self.lib.pkemu_create.restype = C.c_void_p
        self._destroy = self.lib.pkemu_destroy
        self._destroy.argtypes = [C.c_void_p]
        self.desc = _abi.PoseDescC()
        self.desc.settings = settings.to_c()
        self.desc.model = model.to_c()
        self.desc.batch = 1
        err = C.create_string_buffer(256)
        self.h = self.lib.pkemu_create(C.byref(self.desc), err, 256)
        if not self.h:
            raise RuntimeError(err.value.decode())
        v = [C.c_int() for _ in range(4)]
        self.lib.pkemu_dims(C.c_void_p(self.h), *[C.byref(q) for q in v])
        self.n, self.m, self.nnz, self.hnnz = [q.value for q in v]
        caps = (C.c_int * 6)()
        self.lib.pkemu_caps(caps)
        self.ent_cap, self.row_cap, self.touch_cap, self.hess_cap, self.wg, self.max_iterations = list(caps)

    def __del__(self):                     # (on its own names only: at interpreter shutdown a module's globals may be gone before a cached emulation is)
        h, self.h = getattr(self, "h", None), None
        if h:
            self._destroy(h)

    def sparsity(self):
        """(irow, jcol) of jac g in CCS order, (hrow, hcol) of the Hessian's lower triangle in CCS order"""
        ir, jc = np.zeros(self.nnz, np.int32), np.zeros(self.nnz, np.int32)
        hr, hc = np.zeros(self.hnnz, np.int32), np.zeros(self.hnnz, np.int32)
        self.lib.pkemu_sparsity(C.c_void_p(self.h), _ip(ir), _ip(jc), _ip(hr), _ip(hc))
        return ir, jc, hr, hc

    def device_words(self, own=False):
        """col_word, row_word, touch_word, hdiag: the device tables of PoseLayout::fill_kkt_tables, or (own) the emulation's own statement"""
        cw, rw, tw, hd = np.zeros(self.ent_cap, np.int32), np.zeros(self.ent_cap, np.int32), np.zeros(self.touch_cap, np.int32), np.zeros(self.wg, np.int32)
        self.lib.pkemu_device_words(C.c_void_p(self.h), int(own), _ip(cw), _ip(rw), _ip(tw), _ip(hd))
        return {"col_word": cw, "row_word": rw, "touch_word": tw, "hdiag": hd}

    def hdiag(self):
        out = np.zeros(self.n, np.int32)
        self.lib.pkemu_hdiag(C.c_void_p(self.h), _ip(out))
        return out

    def _runs(self, hess, jac):
        hess, jac = _d(hess), _d(jac)
        assert hess.shape == (self.hnnz,) and jac.shape == (self.nnz,)
        return hess, jac

    def _diagonals(self, dx, dc):
        dx, dc = _d(dx), _d(dc)
        assert (dx is None or dx.shape == (self.n,)) and (dc is None or dc.shape == (self.m,))
        return dx, dc

    def times(self, hess, jac, v, w, dx=None, dc=None):
        """Product: K [v; w]; the outputs start as NaN and every store is counted"""
        hess, jac = self._runs(hess, jac)
        dx, dc = self._diagonals(dx, dc)
        v, w = _d(v), _d(w)
        assert v.shape == (self.n,) and w.shape == (self.m,)
        top, bottom = np.full(self.n, np.nan), np.full(self.m, np.nan)
        tw, bw = np.zeros(self.n, np.int32), np.zeros(self.m, np.int32)
        self.lib.pkemu_times(C.c_void_p(self.h), _dp(hess), _dp(jac), _dp(v), _dp(w), _dp(dx), _dp(dc), _dp(top), _ip(tw), _dp(bottom), _ip(bw))
        return Product(top, bottom, tw, bw)

    def diagonal_preconditioner(self, hess, jac, dx=None, dc=None, floor=1e-10):
        """Product: (minv_top, minv_bottom)"""
        hess, jac = self._runs(hess, jac)
        dx, dc = self._diagonals(dx, dc)
        top, bottom = np.full(self.n, np.nan), np.full(self.m, np.nan)
        tw, bw = np.zeros(self.n, np.int32), np.zeros(self.m, np.int32)
        self.lib.pkemu_diag(C.c_void_p(self.h), _dp(hess), _dp(jac), _dp(dx), _dp(dc), C.c_double(floor), _dp(top), _ip(tw), _dp(bottom), _ip(bw))
        return Product(top, bottom, tw, bw)

    def solve(self, hess, jac, rhs_top, rhs_bottom, dx=None, dc=None, minv=None, floor=1e-10, rtol=1e-8, maxiter=400, trace=False):
        """Solution of one pose; minv: None (identity), a pair, or "diagonal" (built inside the solve).  The five outputs start as NaN / -99
        and every store to them is counted.  trace [maxiter, 3]: alfa, beta, phibar of every iteration taken"""
        hess, jac = self._runs(hess, jac)
        dx, dc = self._diagonals(dx, dc)
        bt, bb = _d(rhs_top), _d(rhs_bottom)
        assert bt.shape == (self.n,) and bb.shape == (self.m,)
        build_diag = isinstance(minv, str)
        assert not build_diag or minv == "diagonal"
        mt, mb = (None, None) if (minv is None or build_diag) else (_d(minv[0]), _d(minv[1]))
        assert mt is None or (mt.shape == (self.n,) and mb.shape == (self.m,))
        top, bottom = np.full(self.n, np.nan), np.full(self.m, np.nan)
        tw, bw, sw = np.zeros(self.n, np.int32), np.zeros(self.m, np.int32), np.zeros(3, np.int32)
        it, st, res = C.c_int(-99), C.c_int(-99), C.c_double(float("nan"))
        tr = np.full((maxiter, 3), np.nan) if trace else None
        self.lib.pkemu_solve(C.c_void_p(self.h), _dp(hess), _dp(jac), _dp(bt), _dp(bb), _dp(dx), _dp(dc), _dp(mt), _dp(mb), C.c_int(int(build_diag)), C.c_double(floor),
                             C.c_double(rtol), C.c_int(maxiter), _dp(top), _ip(tw), _dp(bottom), _ip(bw), C.byref(it), C.byref(res), C.byref(st), _ip(sw), _dp(tr))
        return Solution(top, bottom, it.value, res.value, st.value, tw, bw, sw, tr)
