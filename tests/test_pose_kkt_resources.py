"""Occupancy of the three kernels of the pose finder's KKT chain (hipnlp_pose.hip hipnlp_pose_saddle_times_kernel,
hipnlp_pose_saddle_diag_kernel, hipnlp_pose_saddle_solve_kernel), checked on the BUILT library's own code object
(tools/kernel_resources.py): each exists once, has 256 threads, uses no scratch memory (the solve keeps y, r1, r2, w, w2, z, v and minv of
a thread's two elements and the scalar record in registers), and fits at least two workgroups per CU by LDS granules and by registers.
Achieved by the build this was written against: 31 808 B of LDS each (25 granules of 1 280 B: five workgroups per CU by LDS); times 43
VGPRs / 32 SGPRs, diag 28 / 32, solve 110 / 66 (four workgroups per CU by registers).  Their names do not contain "kkt": the resource tests
of the kinodynamic operator and solve count the kernels that do.  CPU only."""
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
NAMES = ("hipnlp_pose_saddle_times_kernel", "hipnlp_pose_saddle_diag_kernel", "hipnlp_pose_saddle_solve_kernel")
PER_CU = 2


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return kernel_resources.kernel_resources(LIB)


@pytest.mark.parametrize("name", NAMES)
def test_each_kernel_is_one_kernel_without_scratch_and_two_workgroups_per_cu(res, name):
    matches = [k for k in res if k.split("(")[0].split("<")[0] == name]
    assert len(matches) == 1, (name, sorted(res))
    r = res[matches[0]]
    print(name, r)
    assert r["wg"] == 256 and r["scratch"] == 0, r
    assert PER_CU * -(-r["lds"] // LDS_GRANULE) * LDS_GRANULE <= LDS_PER_CU, r
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * PER_CU <= VGPR_FILE, r       # a workgroup of four waves: one wave per SIMD


def test_the_kinodynamic_operator_and_solve_keep_their_kernels(res):
    assert not any("kkt" in name for name in NAMES)
    assert len([k for k in res if "kkt" in k]) == 4, sorted(k for k in res if "kkt" in k)
