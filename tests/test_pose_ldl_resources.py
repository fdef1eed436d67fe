"""The two kernels of the pose finder's dense L D L^T (hipnlp_pose.hip hipnlp_pose_saddle_ldl_kernel, hipnlp_pose_saddle_ldl_solve_kernel),
checked on the BUILT library's own code object (tools/kernel_resources.py): each exists once, has a workgroup of 256, 512 or 1 024 threads,
uses no scratch memory and at most the 160 KiB of LDS of one CU; their names do not contain "kkt" (the resource tests of the kinodynamic
operator and solve count the kernels that do); and the eight existing pose kernels (thirteen instantiations) are register for register,
LDS byte for LDS byte what profiles/r14_pose_kkt_resources.txt recorded.  Achieved by the build this was written against:
profiles/r15_pose_ldl_resources.txt.  CPU only."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

LIB = os.path.join(ROOT, "hippopt_amd", "lib", "libhipnlp.so")
NAMES = ("hipnlp_pose_saddle_ldl_kernel", "hipnlp_pose_saddle_ldl_solve_kernel")
LINE = re.compile(r"^(hipnlp_pose_\S+)\s+VGPRs\s+(\d+) \(\+(\d+) AGPRs\)\s+SGPRs\s+(\d+)\s+scratch\s+(\d+) B/lane\s+LDS\s+(\d+) B\s+workgroup\s+(\d+)$")


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return kernel_resources.kernel_resources(LIB)


@pytest.mark.parametrize("name", NAMES)
def test_each_kernel_is_one_kernel_without_scratch_within_one_cu(res, name):
    matches = [k for k in res if k.split("(")[0].split("<")[0] == name]
    assert len(matches) == 1, (name, sorted(res))
    r = res[matches[0]]
    print(name, r)
    assert r["wg"] in (256, 512, 1024) and r["scratch"] == 0 and r["lds"] <= 163840, r
    assert r["lds"] >= 15576 * 8                                                   # the packed triangle of order 176 is static LDS
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * (r["wg"] // 256) <= 512, r       # all waves of the workgroup resident: wg / 256 waves per SIMD


def test_the_existing_pose_kernels_are_what_r14_recorded(res):
    text = open(os.path.join(ROOT, "profiles", "r14_pose_kkt_resources.txt")).read()
    recorded = {}
    for line in text.split("this commit:")[1].split("diff of the complete listings")[0].splitlines():
        m = LINE.match(line.strip())
        if m:
            recorded[m.group(1)] = dict(zip(("vgpr", "agpr", "sgpr", "scratch", "lds", "wg"), (int(v) for v in m.groups()[1:])))
    assert len(recorded) == 13 and len({k.split("<")[0] for k in recorded}) == 8, sorted(recorded)
    for name, want in recorded.items():
        assert name in res, name
        assert {k: res[name][k] for k in want} == want, (name, res[name], want)


def test_the_count_of_kernels_named_kkt_is_unchanged(res):
    assert not any("kkt" in name for name in NAMES)
    assert len([k for k in res if "kkt" in k]) == 4, sorted(k for k in res if "kkt" in k)
