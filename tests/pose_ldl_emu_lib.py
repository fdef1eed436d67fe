"""ctypes access to the TEST-ONLY CPU emulation of the pose finder's dense L D L^T kernels (tests/pose_ldl_emu): assembly, Bunch-Kaufman
factorisation, inertia, regularisation ladder and solves of one pose from stored value runs, and the factorisation at a general order."""
import collections
import ctypes as C

import numpy as np

import emu_build
from emu_build import dp as _dp, ip as _ip
from hippopt_amd import _abi

SO = emu_build.library("pose_ldl_emu")
SRC = emu_build.sources("pose_ldl_emu")

Factored = collections.namedtuple("Factored", "top bottom inertia status tries delta factor pivots top_writes bottom_writes det_not_negative")
General = collections.namedtuple("General", "factor pivots perm kind status inertia det_not_negative")


def build():
    return emu_build.build(SO, SRC)


def _d(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _lib():
    lib = C.CDLL(build())
    lib.plemu_create.restype = C.c_void_p
    lib.plemu_destroy.argtypes = [C.c_void_p]
    return lib


def pack(K):
    """the packed lower triangle, column major, of a symmetric matrix"""
    N = K.shape[0]
    return np.concatenate([K[j:, j] for j in range(N)]).astype(np.float64)


def unpack(N, packed):
    """(L unit lower with the 2x2 blocks' subdiagonal left out, the symmetric block diagonal D is NOT separated): the lower triangle as a matrix"""
    A, at = np.zeros((N, N)), 0
    for j in range(N):
        A[j:, j] = packed[at:at + N - j]
        at += N - j
    return A


def factor_general(K):
    """General of a symmetric matrix (its lower triangle is read)"""
    lib = _lib()
    N = K.shape[0]
    a = pack(np.asarray(K, dtype=np.float64))
    ipiv, perm, kind, out = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(5, np.int32)
    lib.plemu_factor_general(C.c_int(N), _dp(a), _ip(ipiv), _ip(perm), _ip(kind), _ip(out))
    return General(a, ipiv, perm, kind, int(out[0]), tuple(int(v) for v in out[1:4]), int(out[4]))


def solve_general(N, factor, pivots, b):
    lib = _lib()
    x, w = np.full(N, np.nan), np.zeros(N, np.int32)
    lib.plemu_solve_general(C.c_int(N), _dp(_d(factor)), _ip(np.ascontiguousarray(pivots, dtype=np.int32)), _dp(_d(b)), _dp(x), _ip(w))
    assert np.all(w == 1)
    return x


def call_error(which, **kw):
    """the reason pose_ldl.h refuses a call for (None: it does not).  which: "factor" or "solve"; kw: the presence of each pointer (all
    True by default) and nrhs, delta_init, kappa, max_tries"""
    lib = _lib()
    msg = C.create_string_buffer(256)
    p = lambda k: int(bool(kw.get(k, True)))  # noqa: E731
    if which == "factor":
        rc = lib.plemu_factor_call_error(p("hess"), p("jac"), C.c_int(kw.get("nrhs", 1)), p("rhs_top"), p("rhs_bottom"), p("sol_top"), p("sol_bottom"), p("inertia"), p("status"),
                                         C.c_double(kw.get("delta_init", 0.0)), C.c_double(kw.get("kappa", 0.0)), C.c_int(kw.get("max_tries", 0)), p("factor"), p("pivots"),
                                         msg, 256)
    else:
        rc = lib.plemu_solve_call_error(p("factor"), p("pivots"), C.c_int(kw.get("nrhs", 1)), p("rhs_top"), p("rhs_bottom"), p("sol_top"), p("sol_bottom"), msg, 256)
    return msg.value.decode() if rc else None


def order_fits(m):
    return bool(_lib().plemu_order_fits(C.c_int(m)))


class PoseLdlEmu:
    def __init__(self, settings, model):
        self.lib = _lib()
        self._destroy = self.lib.plemu_destroy
        self.desc = _abi.PoseDescC()
        self.desc.settings = settings.to_c()
        self.desc.model = model.to_c()
        self.desc.batch = 1
        err = C.create_string_buffer(256)
        self.h = self.lib.plemu_create(C.byref(self.desc), err, 256)
        if not self.h:
            raise RuntimeError(err.value.decode())
        v = [C.c_int() for _ in range(4)]
        self.lib.plemu_dims(C.c_void_p(self.h), *[C.byref(q) for q in v])
        self.n, self.m, self.nnz, self.hnnz = [q.value for q in v]
        self.N = self.n + self.m
        self.doubles = self.N * (self.N + 1) // 2
        caps = (C.c_int * 6)()
        self.lib.plemu_caps(caps)
        self.max_order, self.max_doubles, self.max_nrhs, self.max_tries, self.hess_cap, self.ent_cap = list(caps)

    def __del__(self):                     # (on its own names only: at interpreter shutdown a module's globals may be gone before a cached emulation is)
        h, self.h = getattr(self, "h", None), None
        if h:
            self._destroy(h)

    def sparsity(self):
        """(irow, jcol) of jac g in CCS order, (hrow, hcol) of the Hessian's lower triangle in CCS order"""
        ir, jc = np.zeros(self.nnz, np.int32), np.zeros(self.nnz, np.int32)
        hr, hc = np.zeros(self.hnnz, np.int32), np.zeros(self.hnnz, np.int32)
        self.lib.plemu_sparsity(C.c_void_p(self.h), _ip(ir), _ip(jc), _ip(hr), _ip(hc))
        return ir, jc, hr, hc

    def device_words(self):
        """hess_at, jac_at: the device table of PoseLayout::fill_ldl_tables"""
        ha, ja = np.zeros(self.hess_cap, np.int32), np.zeros(self.ent_cap, np.int32)
        self.lib.plemu_device_words(C.c_void_p(self.h), _ip(ha), _ip(ja))
        return ha, ja

    def factor(self, hess, jac, dx=None, dc=None, rhs_top=None, rhs_bottom=None, delta_init=0.0, kappa=0.0, max_tries=0, store=True):
        """Factored of one pose; rhs_top [nrhs, 81] / rhs_bottom [nrhs, m] or None (nrhs = 0).  The solutions start as NaN and every
        store is counted."""
        hess, jac, dx, dc = _d(hess), _d(jac), _d(dx), _d(dc)
        assert hess.shape == (self.hnnz,) and jac.shape == (self.nnz,) and (dx is None or dx.shape == (self.n,)) and (dc is None or dc.shape == (self.m,))
        nrhs = 0 if rhs_top is None else int(np.asarray(rhs_top).shape[0])
        bt = _d(rhs_top) if nrhs else np.zeros((0, self.n))
        bb = _d(rhs_bottom) if nrhs else np.zeros((0, self.m))
        assert bt.shape == (nrhs, self.n) and bb.shape == (nrhs, self.m)
        top, bottom = np.full((nrhs, self.n), np.nan), np.full((nrhs, self.m), np.nan)
        tw, bw = np.zeros((nrhs, self.n), np.int32), np.zeros((nrhs, self.m), np.int32)
        inertia, scalars, delta = np.full(3, -99, np.int32), np.full(2, -99, np.int32), np.full(1, np.nan)
        fac = np.full(self.doubles, np.nan) if store else None
        piv = np.full(self.N, -99, np.int32) if store else None
        bad = self.lib.plemu_factor(C.c_void_p(self.h), _dp(hess), _dp(jac), _dp(dx), _dp(dc), C.c_int(nrhs), _dp(bt), _dp(bb), _dp(top), _ip(tw), _dp(bottom), _ip(bw),
                                    _ip(inertia), _ip(scalars), _dp(delta), C.c_double(delta_init), C.c_double(kappa), C.c_int(max_tries), _dp(fac), _ip(piv))
        return Factored(top, bottom, tuple(int(v) for v in inertia), int(scalars[0]), int(scalars[1]), float(delta[0]), fac, piv, tw, bw, int(bad))

    def solve(self, factor, pivots, rhs_top, rhs_bottom):
        """(top [nrhs, 81], bottom [nrhs, m]) from a stored factor and pivot vector"""
        bt, bb = _d(rhs_top), _d(rhs_bottom)
        nrhs = bt.shape[0]
        assert bt.shape == (nrhs, self.n) and bb.shape == (nrhs, self.m)
        top, bottom = np.full((nrhs, self.n), np.nan), np.full((nrhs, self.m), np.nan)
        self.lib.plemu_solve(C.c_void_p(self.h), _dp(_d(factor)), _ip(np.ascontiguousarray(pivots, dtype=np.int32)), C.c_int(nrhs), _dp(bt), _dp(bb), _dp(top), _dp(bottom))
        return top, bottom
