"""Occupancy of the three kernels of the device-resident MINRES solve (hipnlp.hip hipnlp_kkt_minres_apply_kernel, _first_kernel,
_second_kernel), checked on the BUILT library's own code object (tools/kernel_resources.py): 256 threads, no scratch memory, and LDS and
registers for at least two workgroups per CU; and the operator's kernel is still exactly one kernel with the figures it had.  Achieved by
the build this was written against: apply 130 VGPRs / 54 176 B (the operator's 54 144 B and the four doubles of the tree: 43 granules, two
workgroups); first 38 VGPRs / 40 B; second 68 VGPRs / 16 B; hipnlp_kkt_times_kernel 126 VGPRs / 54 144 B as before.  CPU only."""
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
NEW = ("hipnlp_kkt_minres_apply_kernel", "hipnlp_kkt_minres_first_kernel", "hipnlp_kkt_minres_second_kernel")
PER_CU = 2


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return kernel_resources.kernel_resources(LIB)


def named(res, name):
    return [k for k in res if k.split("(")[0].split("<")[0] == name]


@pytest.mark.parametrize("name", NEW)
def test_new_kernel_has_no_scratch_and_two_workgroups_per_cu(res, name):
    matches = named(res, name)
    assert len(matches) == 1, (name, sorted(res))
    r = res[matches[0]]
    print(name, r)
    assert r["wg"] == 256 and r["scratch"] == 0, r
    assert PER_CU * -(-r["lds"] // LDS_GRANULE) * LDS_GRANULE <= LDS_PER_CU, r
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * PER_CU <= VGPR_FILE, r       # a workgroup of four waves: one wave per SIMD


def test_the_operator_is_still_one_kernel(res):
    assert len(named(res, "hipnlp_kkt_times_kernel")) == 1
    assert len([k for k in res if "kkt" in k]) == 1 + len(NEW), sorted(k for k in res if "kkt" in k)
