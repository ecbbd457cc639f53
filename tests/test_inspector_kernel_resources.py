"""The kernel of the inspector's companion library (liblc3gpu_inspector.so: lc3_inspect_views_kernel, lc3gpu_inspect_mixed_views), read
from the BUILT library's code object (no GPU needed): no spilled vector register, no scratch, no static LDS, and at most 64 allocated
vector registers -- the largest allocation that still lets 8 waves share a SIMD (512 registers per lane per SIMD; lc3_inspect_kernel, whose
lane body it shares, has 54 in profiles/views_kernel_resources_after.txt).  And the companion holds nothing of the main library: no kernel
name of that listing occurs in it, so the main library's kernels are the only copies of themselves."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")
AFTER = os.path.join(ROOT, "profiles", "views_kernel_resources_after.txt")


@pytest.fixture(scope="module")
def rows():
    import kernel_resources as KR

    if not os.path.exists(os.path.join(KR.LLVM_BIN, "llvm-objdump")):
        pytest.skip("no llvm-objdump / llvm-readelf under " + KR.LLVM_BIN)
    pkg.build_native()
    return KR.from_library(api.inspector_library_path())


def _listing_names():
    with open(AFTER) as f:
        return [ln.split()[0] for ln in f.read().splitlines()[1:] if len(ln.split()) == 7]


def test_the_companion_holds_one_kernel_within_its_budgets(rows):
    assert [r["name"].count("lc3_inspect_views_kernel") for r in rows] == [1], [r["name"] for r in rows]
    r = rows[0]
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert r.get("private_segment_fixed_size", 0) == 0, r  # no scratch
    assert r.get("sgpr_spill_count", 0) == 0, r
    assert r["group_segment_fixed_size"] == 0, r  # all of its LDS is dynamic: sized per call by the plan
    assert r["vgpr_count"] <= 64, r["vgpr_count"]


def test_no_kernel_of_the_main_library_is_in_the_companion(rows):
    names = _listing_names()
    assert len(names) > 200 and any("lc3_inspect_kernel" in n for n in names)
    mine = [r["name"] for r in rows]
    for n in names:
        assert not any(n in m or m in n for m in mine), n
    with open(api.inspector_library_path(), "rb") as f:
        blob = f.read()
    for n in set(names):
        assert n.encode() not in blob, n


def test_the_main_library_holds_no_kernel_of_the_inspector():
    import kernel_resources as KR

    if not os.path.exists(os.path.join(KR.LLVM_BIN, "llvm-objdump")):
        pytest.skip("no llvm-objdump / llvm-readelf under " + KR.LLVM_BIN)
    assert not [r["name"] for r in KR.from_library(pkg.build_native()) if "inspect_views" in r["name"]]
