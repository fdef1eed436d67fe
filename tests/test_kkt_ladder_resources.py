"""The kernel of the per-knot inertia-correcting ladder (hipnlp.hip hipnlp_kkt_block_ladder_kernel), checked on the BUILT library's own code
object (tools/kernel_resources.py, whose table "kkt_ladder" lists it alone): no scratch memory, the factor kernel's LDS — the packed
triangle of order 189, 143 640 B, and at most 20 200 B beside it — 1 024 threads with every wave resident; and the tables "main" and
"kkt_block" have the name sets of the parent commit (profiles/r16_kkt_block_resources.txt).  Achieved by the build this was written
against: 70 VGPRs, 92 SGPRs, 149 024 B, 1 024 threads.  CPU only."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

LIB = os.path.join(ROOT, "hippopt_amd", "lib", "libhipnlp.so")
KERNEL = "hipnlp_kkt_block_ladder_kernel"
TRIANGLE = 189 * 190 // 2 * 8


@pytest.fixture(scope="module")
def tables():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return {t: kernel_resources.kernel_resources(LIB, table=t) for t in ("main", "kkt_block", "kkt_ladder")}


def test_the_ladder_table_holds_exactly_the_new_kernel(tables):
    assert sorted(tables["kkt_ladder"]) == [KERNEL] == list(kernel_resources.KKT_LADDER)
    assert KERNEL not in tables["main"] and KERNEL not in tables["kkt_block"]


def test_the_ladder_kernel_has_no_scratch_the_factor_kernels_lds_and_all_waves_resident(tables):
    r = tables["kkt_ladder"][KERNEL]
    print(r)
    assert r["scratch"] == 0, r
    assert TRIANGLE == 143640 and TRIANGLE <= r["lds"] <= TRIANGLE + 20200 and r["lds"] <= 163840, r
    assert r["lds"] == tables["kkt_block"]["hipnlp_kkt_block_factor_kernel"]["lds"]          # the same KnotLdlLds
    assert r["wg"] == 1024
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * (r["wg"] // 256) <= 512, r                  # wg / 256 waves per SIMD, all resident


def test_the_other_two_tables_have_the_parent_commits_names(tables):
    text = open(os.path.join(ROOT, "profiles", "r16_kkt_block_resources.txt")).read()
    parent, block = text.split("parent commit:")[1].split("this commit, table kkt_block:")
    names = lambda part: sorted(set(re.findall(r"^\s*(hipnlp_\S+)\s+VGPRs", part, flags=re.M)))  # noqa: E731
    assert len(names(parent)) >= 60
    assert sorted(tables["main"]) == names(parent)
    assert sorted(tables["kkt_block"]) == sorted(kernel_resources.KKT_BLOCK)
    assert set(kernel_resources.KKT_BLOCK) <= set(names(block))
