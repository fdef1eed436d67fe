"""ctypes access to the TEST-ONLY CPU emulation of the pose finder's product kernels (tests/pose_products_emu)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hippopt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libhipnlp_pose_products_emu.so")
SRC = [os.path.join(ROOT, "tests", "pose_products_emu", "pose_products_emu.cpp")] + [
    os.path.join(ROOT, "hippopt_amd", "csrc", f) for f in ("layout.h", "knot_body.h", "knot_lgrad.h", "knot_hvp.h", "nlp_defs.h", "knot_tanh.h", "pose_body.h",
                                                           "pose_hess_body.h", "pose_layout.h", "pose_products.h")] + [
    os.path.join(ROOT, "include", "hipnlp.h")]
GUARD = 8   # NaN words on both sides of every output buffer


def build():
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", SO + ".tmp", SRC[0]])
        os.replace(SO + ".tmp", SO)
    return SO


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def set_wave_order(order):
    """order >= 0: the pose program and the pose Hessian program run every phase wave by wave in that order of the four waves; -1: table order"""
    C.CDLL(build()).ppemu_set_wave_order(int(order))


class Guarded:
    """an output buffer of n doubles between two runs of NaN guard words, with a store counter per element"""

    def __init__(self, n):
        self.raw = np.full(n + 2 * GUARD, np.nan)
        self.out = self.raw[GUARD:GUARD + n]
        self.out[:] = -7.0
        self.writes = np.zeros(n, np.int32)

    def intact(self):
        return bool(np.isnan(self.raw[:GUARD]).all() and np.isnan(self.raw[-GUARD:]).all())


class PoseProductsEmu:
    def __init__(self, settings, model):
        self.lib = C.CDLL(build())
        self.lib.ppemu_create.restype = C.c_void_p
        self.lib.ppemu_map_violations.restype = C.c_long
        self.desc = _abi.PoseDescC()
        self.desc.settings = settings.to_c()
        self.desc.model = model.to_c()
        self.desc.batch = 1
        err = C.create_string_buffer(256)
        self.h = self.lib.ppemu_create(C.byref(self.desc), err, 256)
        if not self.h:
            raise RuntimeError(err.value.decode())
        v = [C.c_int() for _ in range(5)]
        self.lib.ppemu_dims(C.c_void_p(self.h), *[C.byref(q) for q in v])
        self.n, self.m, self.nnz, self.hnnz, self.ntouch = [q.value for q in v]
        caps = (C.c_int * 5)()
        self.lib.ppemu_caps(caps)
        self.ent_cap, self.row_cap, self.touch_cap, self.cnt_max, self.wg = list(caps)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.ppemu_destroy(C.c_void_p(self.h))
            self.h = None

    def map_violations(self):
        return int(self.lib.ppemu_map_violations())

    def sparsity(self):
        """(irow, jcol) of jac g in CCS order, (hrow, hcol) of the Hessian's lower triangle in CCS order"""
        ir, jc = np.zeros(self.nnz, np.int32), np.zeros(self.nnz, np.int32)
        hr, hc = np.zeros(self.hnnz, np.int32), np.zeros(self.hnnz, np.int32)
        self.lib.ppemu_sparsity(C.c_void_p(self.h), _ip(ir), _ip(jc), _ip(hr), _ip(hc))
        return ir, jc, hr, hc

    def tables(self):
        """the directories of PoseLayout::build_product_tables: jcolptr, jrowptr, jrowent, htouchptr, touches (pos, slot, other)"""
        jcolptr, jrowptr, jrowent = np.zeros(self.n + 1, np.int32), np.zeros(self.m + 1, np.int32), np.zeros(self.nnz, np.int32)
        htouchptr = np.zeros(self.n + 1, np.int32)
        tp, ts, to = (np.zeros(self.ntouch, np.int32) for _ in range(3))
        self.lib.ppemu_tables(C.c_void_p(self.h), _ip(jcolptr), _ip(jrowptr), _ip(jrowent), _ip(htouchptr), _ip(tp), _ip(ts), _ip(to))
        return {"jcolptr": jcolptr, "jrowptr": jrowptr, "jrowent": jrowent, "htouchptr": htouchptr, "touch_pos": tp, "touch_slot": ts, "touch_other": to}

    def device_words(self):
        """the device tables the kernels read: col_word, row_word, touch_word, col_dir, row_dir, var_dir"""
        cw, rw, tw = np.zeros(self.ent_cap, np.int32), np.zeros(self.ent_cap, np.int32), np.zeros(self.touch_cap, np.int32)
        cd, rd, vd = (np.zeros(self.wg, np.int32) for _ in range(3))
        self.lib.ppemu_device_words(C.c_void_p(self.h), _ip(cw), _ip(rw), _ip(tw), _ip(cd), _ip(rd), _ip(vd))
        return {"col_word": cw, "row_word": rw, "touch_word": tw, "col_dir": cd, "row_dir": rd, "var_dir": vd}

    def perms(self):
        """(staging index of every CCS position of jac g, native Hessian slot of every CCS position of the Hessian)"""
        js, hp = np.zeros(self.nnz, np.int32), np.zeros(self.hnnz, np.int32)
        self.lib.ppemu_perms(C.c_void_p(self.h), _ip(js), _ip(hp))
        return js, hp

    def eval(self, x, p):
        f = C.c_double()
        grad, g, jac = np.full(self.n, np.nan), np.full(self.m, np.nan), np.full(self.nnz, np.nan)
        self.lib.ppemu_eval(C.c_void_p(self.h), _dp(_d(x)), _dp(_d(p)), C.byref(f), _dp(grad), _dp(g), _dp(jac))
        return f.value, grad, g, jac

    def hess(self, x, p, sigma, lam):
        out = np.full(self.hnnz, np.nan)
        self.lib.ppemu_hess(C.c_void_p(self.h), _dp(_d(x)), _dp(_d(p)), C.c_double(float(sigma)), _dp(_d(lam)), _dp(out))
        return out

    def lagrangian_grad(self, x, p, sigma, lam):
        """Guarded buffer with xbar [n]"""
        lam = _d(lam)
        assert lam.shape == (self.m,)
        b = Guarded(self.n)
        self.lib.ppemu_lgrad(C.c_void_p(self.h), _dp(_d(x)), _dp(_d(p)), C.c_double(float(sigma)), _dp(lam), _dp(b.out), _ip(b.writes))
        return b

    def jac_vec(self, x, p, v, want_dot=True, want_jv=True):
        """(Guarded grad f . v [1] or None, Guarded J v [m] or None)"""
        v = _d(v)
        assert v.shape == (self.n,)
        d, j = (Guarded(1) if want_dot else None), (Guarded(self.m) if want_jv else None)
        null_d, null_i = C.POINTER(C.c_double)(), C.POINTER(C.c_int)()
        self.lib.ppemu_jvp(C.c_void_p(self.h), _dp(_d(x)), _dp(_d(p)), _dp(v), _dp(d.out) if d else null_d, _ip(d.writes) if d else null_i,
                           _dp(j.out) if j else null_d, _ip(j.writes) if j else null_i)
        return d, j

    def hess_vec(self, x, p, sigma, lam, v):
        """Guarded buffer with H v [n]"""
        lam, v = _d(lam), _d(v)
        assert lam.shape == (self.m,) and v.shape == (self.n,)
        b = Guarded(self.n)
        self.lib.ppemu_hvp(C.c_void_p(self.h), _dp(_d(x)), _dp(_d(p)), C.c_double(float(sigma)), _dp(lam), _dp(v), _dp(b.out), _ip(b.writes))
        return b
