"""The Lagrangian-gradient kernel (hipnlp.hip hipnlp_knot_lgrad_kernel) keeps the occupancy of the four-wave callback kernel it derives
from: 256 threads, no scratch, four workgroups per CU on both terrains — checked on the BUILT library's own code objects
(tools/kernel_resources.py).  CPU only."""
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
def test_lagrangian_gradient_kernel_fits_four_workgroups_per_cu(res, terrain):
    r = res["hipnlp_knot_lgrad_kernel<%d>" % terrain]
    assert r["wg"] == 256 and r["scratch"] == 0, r
    assert 4 * (-(-r["lds"] // 1280)) * 1280 <= LDS_PER_CU, r          # (LDS is handed out in granules of 1 280 B)
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * 4 <= VGPR_FILE, r     # four waves per SIMD
