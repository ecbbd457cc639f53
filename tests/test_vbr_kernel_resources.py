"""The kernels of the sized encoder call (lc3gpu_encode_vbr) against the budgets of their uniform twins, read from the BUILT library's code
objects (no GPU needed): the headline view's front and back halves within the register budget tests/test_kernel_resources.py sets for the
uniform ones, no spilled vector register, no more scratch and the same LDS as the twin; the sized packer without scratch."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("lc3-codec_amd")

# sized kernel (48 kHz / 10 ms view) -> (its uniform twin, most vector registers)
TWINS = {
    "lc3_enc_front_vbr_kernelI13lc3_cfg_48k10E": ("lc3_enc_front_kernelI13lc3_cfg_48k10E", 120),
    "lc3_enc_back_vbr_kernelI13lc3_cfg_48k10E": ("lc3_enc_back_kernelI13lc3_cfg_48k10E", 120),
}


@pytest.fixture(scope="module")
def rows():
    import kernel_resources as KR

    if not os.path.exists(os.path.join(KR.LLVM_BIN, "llvm-objdump")):
        pytest.skip("no llvm-objdump / llvm-readelf under " + KR.LLVM_BIN)
    return KR.from_library(pkg.build_native())


def _one(rows, frag):
    hit = [r for r in rows if frag in r["name"]]
    assert len(hit) == 1, (frag, [r["name"] for r in hit])
    return hit[0]


def test_sized_headline_kernels_keep_their_twins_budgets(rows):
    for frag, (twin_frag, most) in TWINS.items():
        r, twin = _one(rows, frag), _one(rows, twin_frag)
        assert r.get("vgpr_spill_count", 0) == 0, (r["name"], r["vgpr_spill_count"])
        assert r["vgpr_count"] <= most, (r["name"], r["vgpr_count"], most)
        assert r.get("private_segment_fixed_size", 0) <= twin.get("private_segment_fixed_size", 0), (r["name"], "scratch")
        assert r["group_segment_fixed_size"] == twin["group_segment_fixed_size"], (r["name"], "LDS")
        assert 4 * r["group_segment_fixed_size"] <= 160 * 1024, (r["name"], "four workgroups per compute unit")


def test_sized_packer_has_no_scratch(rows):
    r = _one(rows, "lc3_pack_vbr_kernel")
    assert r.get("private_segment_fixed_size", 0) == 0 and r.get("vgpr_spill_count", 0) == 0, r
