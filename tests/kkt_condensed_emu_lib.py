"""ctypes access to the TEST-ONLY CPU emulation of the condensed block factorisation of the KKT solve (tests/kkt_condensed_emu), which holds
the block preconditioner's emulation (tests/kkt_block_emu) and everything that one holds."""
import collections
import ctypes as C

import numpy as np

import emu_build
from emu_build import dp as _dp, ip as _ip
from hippopt_amd import _abi
from kkt_block_emu_lib import Block, KktBlockEmu
from kkt_emu_lib import NXK

SO = emu_build.library("kkt_condensed_emu")
SRC = emu_build.sources("kkt_condensed_emu", "kkt_block_emu", "kkt_precond_emu", "kkt_minres_emu", "kkt_emu")

Condensed = collections.namedtuple("Condensed", Block._fields + ("top", "bottom", "top_writes", "bottom_writes"))
KL_OK, KL_NONFINITE = 0, 2


def build():
    return emu_build.build(SO, SRC)


def factor_call_error(*args):
    """kc_factor_call_error of knot_condense.h: (hess, jac, dc, floor, factor, pivots, e, o, inertia, status, minv_top, minv_bottom) -> the
    reason or None"""
    fn = C.CDLL(build()).kcemu_factor_call_error
    fn.argtypes = [C.c_int] * 3 + [C.c_double] + [C.c_int] * 8 + [C.c_char_p, C.c_int]
    msg = C.create_string_buffer(256)
    return msg.value.decode() if fn(*args, msg, 256) else None


class KktCondensedEmu(KktBlockEmu):
    """the condensed factorisation and KktBlockEmu's methods (apply and solve take its record as they take block_factor's), on ONE handle
    of this emulation's library"""

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

    def _runs(self, hess, jac, dx, dc):
        cont = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        hess, jac, dx, dc = cont(hess), cont(jac), cont(dx), cont(dc)
        assert hess.shape == (self.nnz_h,) and jac.shape == (self.nnz,) and (dx is None or dx.shape == (self.n,)) and dc.shape == (self.m,)
        return hess, jac, dx, dc

    def condensed_caps(self):
        """dict(entries_max, rows_max, tables_ok, entries, rows): the two limits of knot_condense.h, whether kc_build_tables accepts this
        layout, and the layout's own figures"""
        out = np.zeros(5, np.int32)
        self.lib.kcemu_caps(C.c_void_p(self.h), _ip(out))
        return dict(entries_max=int(out[0]), rows_max=int(out[1]), tables_ok=bool(out[2]), entries=int(out[3]), rows=int(out[4]))

    def condensed_block(self, k, hess, jac, dc, dx=None):
        """(B_k packed [17955], terms [17955] int32, dc_good) of knot k: the assembled block BEFORE the factorisation and the number of
        fused multiply-adds every element took"""
        hess, jac, dx, dc = self._runs(hess, jac, dx, dc)
        a, terms = np.full(self.doubles, np.nan), np.full(self.doubles, -99, np.int32)
        good = self.lib.kcemu_assemble(C.c_void_p(self.h), C.c_int(k), _dp(hess), _dp(jac), _dp(dx), _dp(dc), _dp(a), _ip(terms))
        return a, terms, bool(good)

    def condensed_block_through_tables(self, k, hess, jac, dc, dx=None):
        """(B_k packed [17955], the six globals' accumulated diagonal [6]) through the DEVICE tables and the device's merge; raises where
        the tables cannot be built or a word of them points outside what the kernel stages"""
        hess, jac, dx, dc = self._runs(hess, jac, dx, dc)
        a, glob = np.full(self.doubles, np.nan), np.full(6, np.nan)
        rc = self.lib.kcemu_assemble_tables(C.c_void_p(self.h), C.c_int(k), _dp(hess), _dp(jac), _dp(dx), _dp(dc), _dp(a), _dp(glob))
        if rc != 1:
            raise RuntimeError("condensation tables: %s" % ("not built" if rc == 0 else "a word outside the staging"))
        return a, glob

    def condensed_factor(self, hess, jac, dc, dx=None, floor=1e-10):
        """Condensed(Block's fields, top [n], bottom [m], the stores counted) of one trajectory: hipnlp_kkt_condensed_factor_device; every
        output starts as a sentinel"""
        hess, jac, dx, dc = self._runs(hess, jac, dx, dc)
        N = self.N
        factor, words = np.full((N, self.doubles), -7.0), np.full((N, NXK), -99, np.int32)
        e, o = np.full((N, NXK), -7.0), np.full((N, NXK), -7.0)
        inertia, status, checks = np.full((N, 3), -99, np.int32), np.full(N, -99, np.int32), np.zeros(2, np.int32)
        top, bottom = np.full(self.n, -7.0), np.full(self.m, -7.0)
        tw, bw = np.zeros(self.n, np.int32), np.zeros(self.m, np.int32)
        self.lib.kcemu_factor(C.c_void_p(self.h), _dp(hess), _dp(jac), _dp(dx), _dp(dc), C.c_double(floor), _dp(factor), _ip(words), _dp(e), _dp(o), _ip(inertia), _ip(status),
                              _dp(top), _dp(bottom), _ip(tw), _ip(bw), _ip(checks))
        return Condensed(factor, words, e, o, inertia, status, int(checks[0]), int(checks[1]), top, bottom, tw, bw)
