"""The kernel of the analyzer's companion library (liblc3gpu_analyzer.so: lc3_analyze_views_kernel, lc3gpu_analyze_mixed_views), read from
the BUILT library's code object (no GPU needed): no spilled vector register, no scratch, no static LDS, and at most 128 allocated vector
registers (lc3_parse_kernel<lc3_cfg_any>, whose lane body it shares, has 109 in profiles/views_kernel_resources_after.txt).  The companion
holds nothing of the main library -- no kernel name of that listing occurs in it -- and neither the main library nor the inspector's
companion holds anything named analyze_views."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")
AFTER = os.path.join(ROOT, "profiles", "views_kernel_resources_after.txt")


def _kr():
    import kernel_resources as KR

    if not os.path.exists(os.path.join(KR.LLVM_BIN, "llvm-objdump")):
        pytest.skip("no llvm-objdump / llvm-readelf under " + KR.LLVM_BIN)
    return KR


@pytest.fixture(scope="module")
def rows():
    KR = _kr()
    pkg.build_native()
    return KR.from_library(api.analyzer_library_path())


def _listing_names():
    with open(AFTER) as f:
        return [ln.split()[0] for ln in f.read().splitlines()[1:] if len(ln.split()) == 7]


def test_the_companion_holds_one_kernel_within_its_budgets(rows):
    assert [r["name"].count("lc3_analyze_views_kernel") for r in rows] == [1], [r["name"] for r in rows]
    r = rows[0]
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert r.get("private_segment_fixed_size", 0) == 0, r  # no scratch
    assert r.get("sgpr_spill_count", 0) == 0, r
    assert r["group_segment_fixed_size"] == 0, r  # all of its LDS is dynamic: sized per call by the plan
    assert r["vgpr_count"] <= 128, r["vgpr_count"]


def test_the_committed_listing_is_the_built_kernel(rows):
    """profiles/analyze_views_kernel_resources.txt is this kernel's row"""
    with open(os.path.join(ROOT, "profiles", "analyze_views_kernel_resources.txt")) as f:
        lines = [ln.split() for ln in f.read().splitlines() if "lc3_analyze_views_kernel" in ln]
    assert len(lines) == 1 and len(lines[0]) == 7
    r = rows[0]
    assert lines[0][0] in r["name"] or r["name"] in lines[0][0]
    assert int(lines[0][1]) == r["vgpr_count"]


def test_no_kernel_of_the_main_library_is_in_the_companion(rows):
    names = _listing_names()
    assert len(names) > 200 and any("lc3_parse_kernel" in n for n in names)
    mine = [r["name"] for r in rows]
    for n in names:
        assert not any(n in m or m in n for m in mine), n
    with open(api.analyzer_library_path(), "rb") as f:
        blob = f.read()
    for n in set(names):
        assert n.encode() not in blob, n
    assert b"lc3_inspect_views_kernel" not in blob


def test_the_main_library_and_the_inspectors_companion_hold_nothing_named_analyze_views():
    KR = _kr()
    main = pkg.build_native()
    for path in (main, api.inspector_library_path()):
        assert not [r["name"] for r in KR.from_library(path) if "analyze_views" in r["name"]], path
        with open(path, "rb") as f:
            assert b"analyze_views_kernel" not in f.read(), path
