"""Occupancy of the one-launch KKT operator kernel (hipnlp.hip hipnlp_kkt_times_kernel), checked on the BUILT library's own code object
(tools/kernel_resources.py): 256 threads, no scratch memory, and two workgroups per CU both by the LDS (handed out in granules of 1 280 B
of 160 KB) and by the registers.  Achieved by the build this was written against: 126 VGPRs / 54 144 B (43 granules: two workgroups, 384 B
past the 42 granules that three would need).  CPU only."""
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
NAME, PER_CU = "hipnlp_kkt_times_kernel", 2


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return kernel_resources.kernel_resources(LIB)


def test_kkt_kernel_has_no_scratch_and_two_workgroups_per_cu(res):
    matches = [k for k in res if k.split("(")[0].split("<")[0] == NAME]
    assert len(matches) == 1, (NAME, sorted(res))
    r = res[matches[0]]
    print(r)
    assert r["wg"] == 256 and r["scratch"] == 0, r
    assert r["lds"] <= 80 * 1024 and PER_CU * -(-r["lds"] // LDS_GRANULE) * LDS_GRANULE <= LDS_PER_CU, r
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * PER_CU <= VGPR_FILE, r       # a workgroup of four waves: one wave per SIMD
