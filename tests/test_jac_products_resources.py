"""Occupancy of the stored-values Jacobian product kernels (hipnlp.hip), checked on the BUILT library's own code objects
(tools/kernel_resources.py): 256 threads, no scratch memory, and the workgroups per CU DESIGN.md §3 states for them — three for
hipnlp_jac_times_kernel (two value blocks, the entry words and three records of v in LDS), six for
hipnlp_jac_transpose_times_kernel (one block, the multipliers, the entry words).  Achieved by the build this was written against:
46 VGPRs / 42 720 B and 42 VGPRs / 25 792 B.  CPU only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

LIB = os.path.join(ROOT, "hippopt_amd", "lib", "libhipnlp.so")
LDS_PER_CU = 160 * 1024
LDS_GRANULE = 1280       # LDS is handed out in granules of 1 280 B
VGPR_FILE = 512          # per SIMD lane (unified VGPR + AGPR file of gfx950)
PER_CU = {"hipnlp_jac_times_kernel": 3, "hipnlp_jac_transpose_times_kernel": 6}


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return kernel_resources.kernel_resources(LIB)


@pytest.mark.parametrize("name", list(PER_CU))
def test_product_kernel_has_no_scratch_and_the_stated_occupancy(res, name):
    matches = [k for k in res if k.split("(")[0].split("<")[0] == name]
    assert len(matches) == 1, (name, sorted(res))
    r = res[matches[0]]
    per_cu = PER_CU[name]
    assert r["wg"] == 256 and r["scratch"] == 0, r
    assert per_cu * -(-r["lds"] // LDS_GRANULE) * LDS_GRANULE <= LDS_PER_CU, r
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * per_cu <= VGPR_FILE, r       # a workgroup of four waves: one wave per SIMD


def test_dot_reduction_kernel_is_one_wave_without_scratch_or_lds(res):
    r = res[[k for k in res if k.startswith("hipnlp_jac_dot_reduce_kernel")][0]]
    assert r["wg"] == 64 and r["scratch"] == 0 and r["lds"] == 0, r
