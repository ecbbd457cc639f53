"""The wave-per-stream kernels of the mixed-list calls (lc3gpu_encode_mixed_list / lc3gpu_decode_mixed_list) against their *_mixed twins,
read from the BUILT library's code objects (no GPU needed).  Each new kernel: no spilled vector register, no more scratch than its twin,
the twin's LDS, at most the twin's vector registers.  The yardstick is the twin as the commit BEFORE the new kernels compiled it
(profiles/mixed_list_kernel_resources_before.txt), not a kernel of this build."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("lc3-codec_amd")
BEFORE = os.path.join(ROOT, "profiles", "mixed_list_kernel_resources_before.txt")

# new kernel (name fragment) -> its twin: the kernels a multi-unit library launches (<name>_all, a body per compile-time view)
TWINS = {
    "lc3_enc_front_mixed_list_kernel_all": "lc3_enc_front_mixed_kernel_all",
    "lc3_enc_back_mixed_list_kernel_all": "lc3_enc_back_mixed_kernel_all",
    "lc3_decode_mixed_list_kernel_all": "lc3_decode_mixed_kernel_all",
    "lc3_decode_mixed_list_late_kernel_all": "lc3_decode_mixed_late_kernel_all",
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


def test_mixed_list_kernels_keep_their_twins_budgets(rows):
    before = _before()
    for frag, twin_frag in TWINS.items():
        r, twin = _one(rows, frag), _one(before, twin_frag)
        assert r.get("vgpr_spill_count", 0) == 0, (r["name"], r["vgpr_spill_count"])
        assert r.get("private_segment_fixed_size", 0) <= twin["private_segment_fixed_size"], (r["name"], "scratch", r["private_segment_fixed_size"])
        assert r["group_segment_fixed_size"] == twin["group_segment_fixed_size"], (r["name"], "LDS", r["group_segment_fixed_size"])
        assert r["vgpr_count"] <= twin["vgpr_count"], (r["name"], r["vgpr_count"], twin["vgpr_count"])
        assert 4 * r["group_segment_fixed_size"] <= 160 * 1024, (r["name"], "four workgroups per compute unit")


def test_the_new_kernels_are_absent_from_the_parent_listing():
    names = [r["name"] for r in _before()]
    for frag in TWINS:
        assert not any(frag in n for n in names), frag

