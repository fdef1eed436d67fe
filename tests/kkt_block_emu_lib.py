"""ctypes access to the TEST-ONLY CPU emulation of the block preconditioner of the KKT solve (tests/kkt_block_emu)."""
import collections
import ctypes as C

import numpy as np

import emu_build
from emu_build import dp as _dp, ip as _ip
from hippopt_amd import _abi
from kkt_emu_lib import NXK
from kkt_minres_emu_lib import Solution
from kkt_precond_emu_lib import KktPrecondEmu

SO = emu_build.library("kkt_block_emu")
SRC = emu_build.sources("kkt_block_emu", "kkt_precond_emu", "kkt_minres_emu", "kkt_emu")

Block = collections.namedtuple("Block", "factor words e o inertia status det_not_negative not_positive_definite")
Applied = collections.namedtuple("Applied", "top bottom top_writes bottom_writes")
PL_ONE, PL_FIRST, PL_SECOND = 0, 1, 2


def build():
    return emu_build.build(SO, SRC)


def caps():
    out = np.zeros(3, np.int32)
    C.CDLL(build()).kbemu_caps(_ip(out))
    return dict(order=int(out[0]), doubles=int(out[1]), entries=int(out[2]))


def word_ipiv(w):
    return (np.asarray(w, np.int64) & 0xffff).astype(np.uint16).view(np.int16).astype(np.int64)


def word_perm(w):
    return (np.asarray(w, np.int64) >> 16) & 0xff


def word_kind(w):
    return (np.asarray(w, np.int64) >> 24) & 3


def call_errors():
    """the three *_call_error functions of knot_ldl.h as python callables returning the reason or None"""
    lib = C.CDLL(build())

    def wrap(fn, types):
        fn.argtypes = types + [C.c_char_p, C.c_int]

        def call(*args):
            msg = C.create_string_buffer(256)
            return msg.value.decode() if fn(*args, msg, 256) else None
        return call
    i, d = C.c_int, C.c_double
    return dict(factor=wrap(lib.kbemu_factor_call_error, [i, d] + [i] * 6), apply=wrap(lib.kbemu_apply_call_error, [i] * 10),
                minres=wrap(lib.kbemu_minres_call_error, [i] * 15 + [d, i, i]))


class KktBlockEmu(KktPrecondEmu):
    """the block factorisation, its apply and the solve with it, beside the diagonal's, the solve's and the operator's emulations
    (KktPrecondEmu's, KktMinresEmu's and KktEmu's methods), on ONE handle of ONE library: this emulation's, which holds the other three"""

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
        self.doubles = NXK * (NXK + 1) // 2

    def block_pattern(self):
        """(at [entries cap] the device table, lrow [nnz_knot], lcol [nnz_knot])"""
        cap = caps()["entries"]
        at, lrow, lcol = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        k = self.lib.kbemu_device_words(C.c_void_p(self.h), _ip(at), _ip(lrow), _ip(lcol))
        return at, lrow[:k], lcol[:k]

    def block_factor(self, hess, dx=None, floor=1e-10):
        """Block(factor [N, 17955], words [N, 189], e, o [N, 189], inertia [N, 3], status [N], two check counts) of one trajectory"""
        hess = np.ascontiguousarray(hess, np.float64)
        dx = None if dx is None else np.ascontiguousarray(dx, np.float64)
        assert hess.shape == (self.nnz_h,) and (dx is None or dx.shape == (self.n,))
        N = self.N
        factor, words = np.full((N, self.doubles), np.nan), np.full((N, NXK), -99, np.int32)
        e, o = np.full((N, NXK), np.nan), np.full((N, NXK), np.nan)
        inertia, status, checks = np.full((N, 3), -99, np.int32), np.full(N, -99, np.int32), np.zeros(2, np.int32)
        self.lib.kbemu_factor(C.c_void_p(self.h), _dp(hess), _dp(dx), C.c_double(floor), _dp(factor), _ip(words), _dp(e), _dp(o), _ip(inertia), _ip(status), _ip(checks))
        return Block(factor, words, e, o, inertia, status, int(checks[0]), int(checks[1]))

    def block_apply(self, blk, minv, r_top, r_bottom):
        """Applied(top [n], bottom [m], writes) = M^-1 [r_top; r_bottom]; the destinations start as NaN and every store is counted"""
        cont = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        mt, mb, r_top, r_bottom = cont(minv[0]), cont(minv[1]), cont(r_top), cont(r_bottom)
        assert mt.shape == r_top.shape == (self.n,) and mb.shape == r_bottom.shape == (self.m,)
        top, bottom = np.full(self.n, np.nan), np.full(self.m, np.nan)
        tw, bw = np.zeros(self.n, np.int32), np.zeros(self.m, np.int32)
        self.lib.kbemu_apply(C.c_void_p(self.h), _dp(cont(blk.factor)), _ip(np.ascontiguousarray(blk.words, np.int32)), _dp(cont(blk.e)), _dp(cont(blk.o)), _dp(mt), _dp(mb),
                             _dp(r_top), _dp(r_bottom), _dp(top), _dp(bottom), _ip(tw), _ip(bw))
        return Applied(top, bottom, tw, bw)

    def block_solve(self, hess, jac, rhs_top, rhs_bottom, blk, minv, dx=None, dc=None, rtol=1e-8, maxiter=200, launched=None):
        """Solution (kkt_minres_emu_lib's, without traces) of one trajectory with the block preconditioner"""
        cont = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        hess, jac, dx, dc, rhs_top, rhs_bottom, mt, mb = cont(hess), cont(jac), cont(dx), cont(dc), cont(rhs_top), cont(rhs_bottom), cont(minv[0]), cont(minv[1])
        assert hess.shape == (self.nnz_h,) and jac.shape == (self.nnz,) and rhs_top.shape == mt.shape == (self.n,) and rhs_bottom.shape == mb.shape == (self.m,)
        launched = maxiter if launched is None else launched
        top, bottom = np.full(self.n, np.nan), np.full(self.m, np.nan)
        tw, bw, sw = np.zeros(self.n, np.int32), np.zeros(self.m, np.int32), np.zeros(3, np.int32)
        it, st, res = C.c_int(-99), C.c_int(-99), C.c_double(float("nan"))
        self.lib.kbemu_solve(C.c_void_p(self.h), _dp(hess), _dp(jac), _dp(dx), _dp(dc), _dp(cont(blk.factor)), _ip(np.ascontiguousarray(blk.words, np.int32)), _dp(cont(blk.e)),
                             _dp(cont(blk.o)), _dp(mt), _dp(mb), _dp(rhs_top), _dp(rhs_bottom), _dp(top), _dp(bottom), C.c_double(rtol), C.c_int(maxiter), C.c_int(launched),
                             C.byref(it), C.byref(res), C.byref(st), _ip(tw), _ip(bw), _ip(sw))
        return Solution(top, bottom, it.value, res.value, st.value, tw, bw, sw, None, None)
