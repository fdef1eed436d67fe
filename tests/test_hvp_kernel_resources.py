"""The fused Hessian-vector kernel (hipnlp.hip hipnlp_knot_hvp_kernel) keeps the occupancy of the compact Hessian kernel it derives from:
256 threads, no scratch, three workgroups per CU by LDS granules and by registers on both terrains; the stored-values kernel uses no
scratch — checked on the BUILT library's own code objects (tools/kernel_resources.py).  CPU only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

LIB = os.path.join(ROOT, "hippopt_amd", "lib", "libhipnlp.so")
LDS_PER_CU = 160 * 1024
VGPR_FILE = 512          # per SIMD lane (unified VGPR + AGPR file of gfx950)


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    return kernel_resources.kernel_resources(LIB)


@pytest.mark.parametrize("terrain", [0, 1])
def test_fused_kernel_fits_three_workgroups_per_cu(res, terrain):
    r = res["hipnlp_knot_hvp_kernel<%d>" % terrain]
    assert r["wg"] == 256 and r["scratch"] == 0, r
    assert 3 * (-(-r["lds"] // 1280)) * 1280 <= LDS_PER_CU, r          # (LDS is handed out in granules of 1 280 B)
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * 3 <= VGPR_FILE, r     # three waves per SIMD
    assert r["lds"] <= res["hipnlp_knot_hess_kernel<%d,1>" % terrain]["lds"], r   # no more LDS than the compact Hessian kernel


def test_stored_values_kernel_uses_no_scratch(res):
    r = res["hipnlp_hess_times_kernel"]
    assert r["wg"] == 256 and r["scratch"] == 0, r
