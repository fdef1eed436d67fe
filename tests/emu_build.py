"""What the ctypes wrappers of the TEST-ONLY stored-values emulations share (jprod_emu_lib, kkt_emu_lib, kkt_minres_emu_lib,
kkt_precond_emu_lib): where things are, the one-file g++ build with its staleness check, and the ctypes pointer helpers."""
import ctypes as C
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every header an emulation may reach: a new one under csrc/ cannot be forgotten
DEPS = sorted(glob.glob(os.path.join(ROOT, "hippopt_amd", "csrc", "*.h"))) + [os.path.join(ROOT, "include", "hipnlp.h"),
                                                                               os.path.join(ROOT, "tests", "values_stage_emu.h")]
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-variable", "-Wno-missing-field-initializers"]


def library(name):
    """tests/_build/libhipnlp_<name>.so"""
    return os.path.join(ROOT, "tests", "_build", "libhipnlp_%s.so" % name)


def sources(*names):
    """tests/<name>/<name>.cpp for each name: the file that is compiled first, then the emulations it includes"""
    return [os.path.join(ROOT, "tests", n, n + ".cpp") for n in names]


def build(so, src):
    """compile src[0] into `so` when `so` is older than any of src or DEPS; returns `so`"""
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in list(src) + DEPS):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++"] + FLAGS + ["-o", so + ".tmp", src[0]])
        os.replace(so + ".tmp", so)
    return so


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int)) if a is not None else None


def lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_long))
