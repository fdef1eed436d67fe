"""The kernel of the condensed block factorisation (hipnlp.hip hipnlp_kkt_condensed_factor_kernel), checked on the BUILT library's own code
object (tools/kernel_resources.py, whose table "kkt_condensed" lists it alone): no scratch memory, its LDS — the packed triangle of order
189, 143 640 B, and the staging behind it — within the 160 KB one workgroup can have, 1 024 threads with every wave resident; and every
kernel that existed before has the parent commit's registers, scratch, LDS and workgroup size, in the table it was in
(profiles/r18_kkt_condensed_resources.txt).  Achieved by the build this was written against: 52 VGPRs, 80 SGPRs, 163 792 B.  CPU only."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

LIB = os.path.join(ROOT, "hippopt_amd", "lib", "libhipnlp.so")
KERNEL = "hipnlp_kkt_condensed_factor_kernel"
TRIANGLE = 189 * 190 // 2 * 8
LINE = re.compile(r"^(hipnlp_\S+)\s+VGPRs\s+(\d+) \(\+(\d+) AGPRs\)\s+SGPRs\s+(\d+)\s+scratch\s+(\d+) B/lane\s+LDS\s+(\d+) B\s+workgroup\s+(\d+)$", re.M)


@pytest.fixture(scope="module")
def tables():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return {t: kernel_resources.kernel_resources(LIB, table=t) for t in ("main", "kkt_block", "kkt_ladder", "kkt_condensed")}


def test_the_condensed_table_holds_exactly_the_new_kernel(tables):
    assert sorted(tables["kkt_condensed"]) == [KERNEL] == list(kernel_resources.KKT_CONDENSED)
    assert all(KERNEL not in tables[t] for t in ("main", "kkt_block", "kkt_ladder"))


def test_the_new_kernel_has_no_scratch_and_its_lds_fits_one_workgroup(tables):
    r = tables["kkt_condensed"][KERNEL]
    print(r)
    assert r["scratch"] == 0, r
    assert TRIANGLE == 143640 and TRIANGLE < r["lds"] <= 160 * 1024, r
    assert r["wg"] == 1024
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * (r["wg"] // 256) <= 512, r                  # wg / 256 waves per SIMD, all resident


def test_every_kernel_that_existed_before_has_the_parent_commits_resources(tables):
    text = open(os.path.join(ROOT, "profiles", "r18_kkt_condensed_resources.txt")).read()
    parent = text.split("parent commit:")[1].split("this commit, table kkt_condensed:")[0]
    want = {m[0]: dict(vgpr=int(m[1]), agpr=int(m[2]), sgpr=int(m[3]), scratch=int(m[4]), lds=int(m[5]), wg=int(m[6])) for m in LINE.findall(parent)}
    assert len(want) >= 67
    got = {}
    for t in ("main", "kkt_block", "kkt_ladder"):
        got.update(tables[t])
    assert sorted(got) == sorted(want)                                           # no kernel left, none came into the old tables
    for name in sorted(want):
        assert got[name] == want[name], (name, got[name], want[name])
    assert sorted(tables["kkt_block"]) == sorted(kernel_resources.KKT_BLOCK) and sorted(tables["kkt_ladder"]) == sorted(kernel_resources.KKT_LADDER)
