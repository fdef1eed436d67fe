"""ctypes access to the TEST-ONLY CPU emulation of the device-built diagonal preconditioner of the KKT solve (tests/kkt_precond_emu)."""
import collections
import ctypes as C

import numpy as np

import emu_build
from emu_build import dp as _dp, ip as _ip
from hippopt_amd import _abi
from kkt_emu_lib import NXK
from kkt_minres_emu_lib import KktMinresEmu

SO = emu_build.library("kkt_precond_emu")
SRC = emu_build.sources("kkt_precond_emu", "kkt_minres_emu", "kkt_emu")

Diagonal = collections.namedtuple("Diagonal", "top bottom top_writes bottom_writes")


def build():
    return emu_build.build(SO, SRC)


class KktPrecondEmu(KktMinresEmu):
    """building the diagonal, the solve and the operator's emulation (KktMinresEmu's and KktEmu's methods) on ONE handle of ONE library:
    this emulation's, which holds the other two"""

    def __init__(self, settings, model, detect_simple_bounds=False, jac_varying_first=False):
        # (KktMinresEmu.__init__ with this library in place of its own: the handle, and __del__, are the base class's)
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

    def diag_positions(self):
        """[NXK] the block position of every knot-record variable's diagonal entry of the Hessian, -1: none (HessLayout::hv_diag)"""
        pos = np.zeros(NXK, np.int32)
        self.lib.kpcemu_diag_positions(C.c_void_p(self.h), _ip(pos))
        return pos

    def diagonal_preconditioner(self, hess, jac, dx=None, dc=None, floor=1e-10):
        """Diagonal(top [n], bottom [m], top_writes, bottom_writes) of one trajectory, the device kernel's way; the destinations start as
        NaN and every store to them is counted"""
        cont = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        hess, jac, dx, dc = cont(hess), cont(jac), cont(dx), cont(dc)
        assert hess.shape == (self.nnz_h,) and jac.shape == (self.nnz,)
        assert (dx is None or dx.shape == (self.n,)) and (dc is None or dc.shape == (self.m,))
        top, bottom = np.full(self.n, np.nan), np.full(self.m, np.nan)
        tw, bw = np.zeros(self.n, np.int32), np.zeros(self.m, np.int32)
        self.lib.kpcemu_build(C.c_void_p(self.h), _dp(hess), _dp(jac), _dp(dx), _dp(dc), C.c_double(floor), _dp(top), _dp(bottom), _ip(tw), _ip(bw))
        return Diagonal(top, bottom, tw, bw)
