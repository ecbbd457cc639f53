"""The seven kernels the multi-channel items calls add (lc3gpu_encode_mixed_mc_items / lc3gpu_decode_mixed_mc_items) against the items
kernels they are twins of, read from the BUILT library's code objects (no GPU needed).  Each mc kernel: no spilled vector register, no
more scratch, LDS or vector registers than its items twin.  The yardstick is the twin as the commit BEFORE the mc kernels compiled it
(profiles/mc_items_kernel_resources_before.txt), not a kernel of this build."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("lc3-codec_amd")
BEFORE = os.path.join(ROOT, "profiles", "mc_items_kernel_resources_before.txt")

TWINS = {
    "lc3_enc_front_mc_items_kernel_all": "lc3_enc_front_items_kernel_all",
    "lc3_pack_mc_items_kernel_all": "lc3_pack_items_kernel_all",
    "lc3_pack_pc_mc_items_kernel_all": "lc3_pack_pc_items_kernel_all",
    "lc3_parse_mc_items_kernel_all": "lc3_parse_items_kernel_all",
    "lc3_parse_pc_mc_items_kernel_all": "lc3_parse_pc_items_kernel_all",
    "lc3_decode_mc_items_kernel_all": "lc3_decode_items_kernel_all",
    "lc3_decode_mc_items_late_kernel_all": "lc3_decode_items_late_kernel_all",
}


def _before():
    rows = []
    with open(BEFORE) as f:
        for ln in f.read().splitlines()[1:]:
            w = ln.split()
            if len(w) == 7:
                rows.append({"name": w[0], "vgpr_count": int(w[1]), "sgpr_count": int(w[2]), "group_segment_fixed_size": int(w[3]),
                             "private_segment_fixed_size": int(w[4]), "vgpr_spill_count": int(w[5]), "sgpr_spill_count": int(w[6])})
    return rows


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


def test_mc_items_kernels_keep_their_twins_budgets(rows):
    before = _before()
    for frag, twin_frag in TWINS.items():
        r, twin = _one(rows, frag), _one(before, twin_frag)
        assert r.get("vgpr_spill_count", 0) == 0, (r["name"], r["vgpr_spill_count"])
        assert r.get("private_segment_fixed_size", 0) <= twin["private_segment_fixed_size"], (r["name"], "scratch", r["private_segment_fixed_size"])
        assert r["group_segment_fixed_size"] <= twin["group_segment_fixed_size"], (r["name"], "LDS", r["group_segment_fixed_size"])
        assert r["vgpr_count"] <= twin["vgpr_count"], (r["name"], r["vgpr_count"], twin["vgpr_count"])


def test_the_mc_items_kernels_are_absent_from_the_parent_listing():
    names = [r["name"] for r in _before()]
    assert names and not any("_mc_items_" in n for n in names)
