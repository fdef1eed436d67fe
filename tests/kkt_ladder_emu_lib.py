"""ctypes access to the TEST-ONLY CPU emulation of the per-knot inertia-correcting ladder of the block factorisation
(tests/kkt_ladder_emu), which holds the block preconditioner's emulation (tests/kkt_block_emu) and everything that one holds."""
import collections
import ctypes as C

import numpy as np

import emu_build
from emu_build import dp as _dp, ip as _ip
from hippopt_amd import _abi
from kkt_block_emu_lib import Block, KktBlockEmu
from kkt_emu_lib import NXK

SO = emu_build.library("kkt_ladder_emu")
SRC = emu_build.sources("kkt_ladder_emu", "kkt_block_emu", "kkt_precond_emu", "kkt_minres_emu", "kkt_emu")

Ladder = collections.namedtuple("Ladder", Block._fields + ("delta", "tries"))
Try = collections.namedtuple("Try", "factor words e o inertia status")
KL_OK, KL_NONFINITE, KL_EXHAUSTED = 0, 2, 3


def build():
    return emu_build.build(SO, SRC)


def caps():
    out = np.zeros(4, np.int32)
    C.CDLL(build()).klemu_caps(_ip(out))
    return dict(max_tries=int(out[0]), ok=int(out[1]), nonfinite=int(out[2]), exhausted=int(out[3]))


def ladder_call_error(*args):
    """kl_ladder_call_error of knot_ldl.h: (hess, floor, delta_init, kappa, max_tries, factor, pivots, e, o, inertia, status, delta, tries) ->
    the reason or None"""
    fn = C.CDLL(build()).klemu_ladder_call_error
    fn.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double] + [C.c_int] * 9 + [C.c_char_p, C.c_int]
    msg = C.create_string_buffer(256)
    return msg.value.decode() if fn(*args, msg, 256) else None


def next_delta(t, delta, delta_init, kappa):
    """pl_next_delta in IEEE doubles: delta of try t >= 1 from the delta of try t - 1"""
    return float(delta_init) if t == 1 else float(np.float64(delta) * np.float64(kappa))


class KktLadderEmu(KktBlockEmu):
    """the ladder, one factorisation at an explicit delta, and KktBlockEmu's methods, on ONE handle of this emulation's library"""

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

    def _run(self, hess, dx):
        hess = np.ascontiguousarray(hess, np.float64)
        dx = None if dx is None else np.ascontiguousarray(dx, np.float64)
        assert hess.shape == (self.nnz_h,) and (dx is None or dx.shape == (self.n,))
        return hess, dx

    def factor_at(self, k, hess, dx=None, floor=1e-10, delta=None):
        """Try(factor [17955], words / e / o [189], inertia [3], status) of ONE factorisation of knot k: delta None is try 0's assembly,
        H_k + dx_k; a number is (H_cc + dx_c) + delta on the diagonal"""
        hess, dx = self._run(hess, dx)
        factor, words = np.full(self.doubles, np.nan), np.full(NXK, -99, np.int32)
        e, o = np.full(NXK, np.nan), np.full(NXK, np.nan)
        inertia, status = np.full(3, -99, np.int32), np.full(1, -99, np.int32)
        self.lib.klemu_factor_at(C.c_void_p(self.h), C.c_int(k), _dp(hess), _dp(dx), C.c_double(floor), C.c_int(delta is not None), C.c_double(0.0 if delta is None else delta),
                                 _dp(factor), _ip(words), _dp(e), _dp(o), _ip(inertia), _ip(status))
        return Try(factor, words, e, o, inertia, int(status[0]))

    def block_ladder(self, hess, dx=None, floor=1e-10, delta_init=1e-4, kappa=8.0, max_tries=16):
        """Ladder(Block's fields, delta [N], tries [N]) of one trajectory: hipnlp_kkt_block_ladder_device"""
        hess, dx = self._run(hess, dx)
        N = self.N
        factor, words = np.full((N, self.doubles), np.nan), np.full((N, NXK), -99, np.int32)
        e, o = np.full((N, NXK), np.nan), np.full((N, NXK), np.nan)
        inertia, status, checks = np.full((N, 3), -99, np.int32), np.full(N, -99, np.int32), np.zeros(2, np.int32)
        delta, tries = np.full(N, np.nan), np.full(N, -99, np.int32)
        self.lib.klemu_ladder(C.c_void_p(self.h), _dp(hess), _dp(dx), C.c_double(floor), C.c_double(delta_init), C.c_double(kappa), C.c_int(max_tries), _dp(factor), _ip(words),
                              _dp(e), _dp(o), _ip(inertia), _ip(status), _dp(delta), _ip(tries), _ip(checks))
        return Ladder(factor, words, e, o, inertia, status, int(checks[0]), int(checks[1]), delta, tries)

    def convexified_dx(self, dx, delta):
        """dx + delta_k on knot k's 189 variables, the six globals untouched (dx None: zeros) — KKTValues.convexify's step 2"""
        out = np.zeros(self.n) if dx is None else np.array(dx, np.float64)
        out[:NXK * self.N] += np.repeat(np.asarray(delta, np.float64), NXK)
        return out
