"""Occupancy of the kernel that builds the diagonal preconditioner of the KKT solve (hipnlp.hip hipnlp_saddle_diag_kernel), checked on the
BUILT library's own code object (tools/kernel_resources.py): one kernel, 256 threads, no scratch memory, and LDS and registers for at
least two workgroups per CU.  Achieved by the build this was written against: 76 VGPRs, 48 SGPRs, 42 688 B of LDS (34 granules of
1 280 B: three workgroups per CU by LDS).  Its name does not contain "kkt": the operator's and the solve's resource tests count the
kernels that do.  CPU only."""
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
NAME = "hipnlp_saddle_diag_kernel"
PER_CU = 2


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return kernel_resources.kernel_resources(LIB)


def named(res, name):
    return [k for k in res if k.split("(")[0].split("<")[0] == name]


def test_the_kernel_is_one_kernel_without_scratch_and_two_workgroups_per_cu(res):
    matches = named(res, NAME)
    assert len(matches) == 1, (NAME, sorted(res))
    r = res[matches[0]]
    print(NAME, r)
    assert r["wg"] == 256 and r["scratch"] == 0, r
    assert PER_CU * -(-r["lds"] // LDS_GRANULE) * LDS_GRANULE <= LDS_PER_CU, r
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * PER_CU <= VGPR_FILE, r       # a workgroup of four waves: one wave per SIMD
    assert r["lds"] <= 54144, r                                               # no more than the operator it shares a grid with


def test_the_operator_and_the_solve_keep_their_kernels(res):
    assert "kkt" not in NAME
    assert len([k for k in res if "kkt" in k]) == 4, sorted(k for k in res if "kkt" in k)
