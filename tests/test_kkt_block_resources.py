"""The three kernels of the block preconditioner of the KKT solve (hipnlp.hip hipnlp_kkt_block_factor_kernel, hipnlp_kkt_block_apply_kernel,
hipnlp_kkt_minres_block_first_kernel), checked on the BUILT library's own code object (tools/kernel_resources.py, whose table "kkt_block"
lists them; its main table lists every other kernel, as before): the factor kernel has no scratch memory and at most the 160 KiB of LDS of
one CU, of which the packed triangle of order 189 is 143 640 B and the rest at most 20 200 B; the block first kernel and the apply kernel
have no scratch memory; and every kernel that existed before has the registers, scratch memory and LDS that
profiles/r16_kkt_block_resources.txt recorded for the parent commit.  Achieved by the build this was written against: factor 48 VGPRs /
149 024 B / 1 024 threads, apply 92 VGPRs / 0 B, block first 106 VGPRs / 3 112 B.  CPU only."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

LIB = os.path.join(ROOT, "hippopt_amd", "lib", "libhipnlp.so")
LINE = re.compile(r"^(hipnlp_\S+)\s+VGPRs\s+(\d+) \(\+(\d+) AGPRs\)\s+SGPRs\s+(\d+)\s+scratch\s+(\d+) B/lane\s+LDS\s+(\d+) B\s+workgroup\s+(\d+)$")
TRIANGLE = 189 * 190 // 2 * 8


@pytest.fixture(scope="module")
def tables():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return kernel_resources.kernel_resources(LIB), kernel_resources.kernel_resources(LIB, table="kkt_block")


def test_the_block_table_has_the_three_kernels_once_each(tables):
    main, block = tables
    assert sorted(block) == sorted(kernel_resources.KKT_BLOCK), sorted(block)
    assert not set(block) & set(main)


def test_the_factor_kernel_has_no_scratch_and_fits_one_cu(tables):
    r = tables[1]["hipnlp_kkt_block_factor_kernel"]
    print(r)
    assert r["scratch"] == 0 and r["lds"] <= 163840, r
    assert TRIANGLE == 143640 and TRIANGLE <= r["lds"] <= TRIANGLE + 20200, r       # the packed triangle is static LDS; what lies beside it
    assert r["wg"] == 1024                                                         # the pose LDL kernel's thread count
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 * (r["wg"] // 256) <= 512, r       # all waves of the workgroup resident: wg / 256 waves per SIMD


@pytest.mark.parametrize("name", ["hipnlp_kkt_minres_block_first_kernel", "hipnlp_kkt_block_apply_kernel"])
def test_the_first_wave_kernels_have_no_scratch(tables, name):
    r = tables[1][name]
    print(name, r)
    assert r["scratch"] == 0 and r["wg"] == 256, r
    assert (r["vgpr"] + r["agpr"] + 7) // 8 * 8 <= 512, r


def test_every_kernel_that_existed_before_is_what_the_parent_commit_had(tables):
    main = tables[0]
    text = open(os.path.join(ROOT, "profiles", "r16_kkt_block_resources.txt")).read()
    recorded = {}
    for line in text.split("parent commit:")[1].split("this commit, table kkt_block:")[0].splitlines():
        m = LINE.match(line.strip())
        if m:
            recorded[m.group(1)] = dict(zip(("vgpr", "agpr", "sgpr", "scratch", "lds", "wg"), (int(v) for v in m.groups()[1:])))
    assert len(recorded) >= 60 and "hipnlp_kkt_minres_first_kernel" in recorded and "hipnlp_pose_saddle_ldl_kernel" in recorded, len(recorded)
    assert sorted(main) == sorted(recorded), sorted(set(main) ^ set(recorded))
    for name, want in recorded.items():
        assert {k: main[name][k] for k in want} == want, (name, main[name], want)
