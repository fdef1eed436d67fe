"""Occupancy of the pose finder's product kernels (hipnlp_pose.hip), checked on the BUILT library's own code objects
(tools/kernel_resources.py) as tests/test_kernel_resources.py checks the kernels they derive from: each keeps the workgroups per CU of
its parent kernel — the first-order kernels five on the planar terrain and four on the smooth steps (hipnlp_pose_kernel), the
Hessian-vector kernel five and three (hipnlp_pose_hess_kernel) — with 256 threads and no scratch memory.  Achieved by the build this was
written against: lgrad 94 / 126 VGPRs, jvp 94 / 124, hvp 90 / 154 (planar / steps); LDS that of the parent kernel to the byte.  CPU only."""
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
PER_CU = {"lgrad": (5, 4), "jvp": (5, 4), "hvp": (5, 3)}   # workgroups per CU: (planar terrain, smooth steps)


def _granule(v):         # the allocation granularity of the register file is 8
    return (v + 7) // 8 * 8


def _lds_granules(b):
    return -(-b // LDS_GRANULE)


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    return kernel_resources.kernel_resources(LIB)


@pytest.mark.parametrize("terrain", [0, 1])
@pytest.mark.parametrize("kind", ["lgrad", "jvp", "hvp"])
def test_product_kernel_keeps_the_occupancy_of_its_parent(res, kind, terrain):
    r = res["hipnlp_pose_%s_kernel<%d>" % (kind, terrain)]
    per_cu = PER_CU[kind][terrain]
    assert r["wg"] == 256 and r["scratch"] == 0, r
    assert per_cu * _lds_granules(r["lds"]) * LDS_GRANULE <= LDS_PER_CU, r
    assert _granule(r["vgpr"] + r["agpr"]) * per_cu <= VGPR_FILE, r       # a workgroup of four waves: one wave per SIMD


@pytest.mark.parametrize("terrain", [0, 1])
def test_hessian_vector_kernel_needs_no_more_lds_than_the_hessian_kernel(res, terrain):
    """touch words and v lie on the knot scratch, which is dead when they arrive: no LDS of their own (one granule of slack)"""
    r, h = res["hipnlp_pose_hvp_kernel<%d>" % terrain], res["hipnlp_pose_hess_kernel<%d>" % terrain]
    assert r["lds"] <= h["lds"] + LDS_GRANULE, (r, h)
