"""Every kernel the items calls launch (lc3gpu_encode_mixed_items / lc3gpu_decode_mixed_items) against the kernel it is a twin of, read from
the BUILT library's code objects (no GPU needed).  Each items kernel: no spilled vector register, no more scratch, LDS or vector registers
than its twin.  The yardstick is the twin as the commit BEFORE the items kernels compiled it
(profiles/items_kernel_resources_before.txt), not a kernel of this build."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("lc3-codec_amd")
BEFORE = os.path.join(ROOT, "profiles", "items_kernel_resources_before.txt")

# items kernel (name fragment) -> its twin in the parent's listing: the mixed-list twin where the kernel finds a stream's state, else the
# mixed kernel (the lane-per-frame encoder kernels have no <name>_all form: they live in the main unit)
TWINS = {
    "lc3_enc_front_items_kernel_all": "lc3_enc_front_mixed_list_kernel_all",
    "lc3_sns_vq_items_kernel_all": "lc3_sns_vq_mixed_kernel",
    "lc3_enc_back_items_kernel_all": "lc3_enc_back_mixed_list_kernel_all",
    "lc3_pack_items_kernel_all": "lc3_pack_mixed_kernel",
    "lc3_pack_pc_items_kernel_all": "lc3_pack_pc_mixed_kernel",
    "lc3_parse_items_kernel_all": "lc3_parse_mixed_kernel_all",
    "lc3_parse_pc_items_kernel_all": "lc3_parse_pc_mixed_kernel_all",
    "lc3_recon_items_kernel_all": "lc3_recon_mixed_kernel_all",
    "lc3_tns_items_kernel_all": "lc3_tns_mixed_kernel_all",
    "lc3_decode_items_kernel_all": "lc3_decode_mixed_list_kernel_all",
    "lc3_decode_items_late_kernel_all": "lc3_decode_mixed_list_late_kernel_all",
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


def test_items_kernels_keep_their_twins_budgets(rows):
    before = _before()
    for frag, twin_frag in TWINS.items():
        r, twin = _one(rows, frag), _one(before, twin_frag)
        assert r.get("vgpr_spill_count", 0) == 0, (r["name"], r["vgpr_spill_count"])
        assert r.get("private_segment_fixed_size", 0) <= twin["private_segment_fixed_size"], (r["name"], "scratch", r["private_segment_fixed_size"])
        assert r["group_segment_fixed_size"] <= twin["group_segment_fixed_size"], (r["name"], "LDS", r["group_segment_fixed_size"])
        assert r["vgpr_count"] <= twin["vgpr_count"], (r["name"], r["vgpr_count"], twin["vgpr_count"])


def test_the_items_kernels_are_absent_from_the_parent_listing():
    names = [r["name"] for r in _before()]
    assert not any("_items_" in n for n in names)


def test_no_kernel_of_the_parent_changed(rows):
    """the items kernels are additions: every row of the parent's listing is in this build's, figure for figure (a name may occur once per
    translation unit: rows are counted)"""
    from collections import Counter

    keys = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
    row = lambda r: (r["name"][:100],) + tuple(r.get(k, 0) for k in keys)  # (the listing prints 100 characters of a name)
    now, before = Counter(row(r) for r in rows), Counter(row(r) for r in _before())
    assert not before - now, sorted(before - now)
    assert all("_items_" in r[0] for r in now - before), sorted(now - before)
