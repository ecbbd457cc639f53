"""The seven kernels the views calls add (lc3gpu_encode_mixed_views / lc3gpu_decode_mixed_views) against the mc-items kernels they are
twins of, read from the BUILT library's code objects (no GPU needed).  Each view kernel: no spilled vector register, no more scratch, LDS
or vector registers than its mc twin.  The yardstick is the twin as the commit BEFORE the view kernels compiled it
(profiles/views_kernel_resources_before.txt), not a kernel of this build; and every kernel of that listing is in this build with the
figures it had: no existing kernel changed."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("lc3-codec_amd")
BEFORE = os.path.join(ROOT, "profiles", "views_kernel_resources_before.txt")
FIGURES = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")

TWINS = {
    "lc3_enc_front_view_items_kernel_all": "lc3_enc_front_mc_items_kernel_all",
    "lc3_pack_view_items_kernel_all": "lc3_pack_mc_items_kernel_all",
    "lc3_pack_pc_view_items_kernel_all": "lc3_pack_pc_mc_items_kernel_all",
    "lc3_parse_view_items_kernel_all": "lc3_parse_mc_items_kernel_all",
    "lc3_parse_pc_view_items_kernel_all": "lc3_parse_pc_mc_items_kernel_all",
    "lc3_decode_view_items_kernel_all": "lc3_decode_mc_items_kernel_all",
    "lc3_decode_view_items_late_kernel_all": "lc3_decode_mc_items_late_kernel_all",
}


def _before():
    rows = []
    with open(BEFORE) as f:
        for ln in f.read().splitlines()[1:]:
            w = ln.split()
            if len(w) == 7:
                rows.append(dict(zip(("name",) + FIGURES, [w[0]] + [int(x) for x in w[1:]])))
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


def test_view_kernels_keep_their_twins_budgets(rows):
    before = _before()
    for frag, twin_frag in TWINS.items():
        r, twin = _one(rows, frag), _one(before, twin_frag)
        assert r.get("vgpr_spill_count", 0) == 0, (r["name"], r["vgpr_spill_count"])
        assert r.get("private_segment_fixed_size", 0) <= twin["private_segment_fixed_size"], (r["name"], "scratch", r["private_segment_fixed_size"])
        assert r["group_segment_fixed_size"] <= twin["group_segment_fixed_size"], (r["name"], "LDS", r["group_segment_fixed_size"])
        assert r["vgpr_count"] <= twin["vgpr_count"], (r["name"], r["vgpr_count"], twin["vgpr_count"])


def test_every_kernel_of_the_parent_listing_is_unchanged_and_only_the_view_kernels_are_new(rows):
    """as multisets of (name, figures): a kernel template instantiated in several translation units appears once per unit"""
    from collections import Counter

    row = lambda r: (r["name"],) + tuple(r.get(k, 0) for k in FIGURES)
    before, now = Counter(row(r) for r in _before()), Counter(row(r) for r in rows)
    assert sum(before.values()) > 200
    gone = before - now
    assert not gone, "kernels of the parent's listing that are missing or compile differently: %s" % sorted(gone)[:5]
    new = sorted(r[0] for r in (now - before).elements())
    assert len(new) == len(TWINS) and all(sum(frag in n for n in new) == 1 for frag in TWINS), new


def test_the_view_kernels_are_absent_from_the_parent_listing():
    names = [r["name"] for r in _before()]
    assert names and not any("_view_items_" in n for n in names)
