"""The kernel of the meter's companion library (liblc3gpu_meter.so: lc3_level_views_kernel, lc3gpu_measure_mixed_views), read from the BUILT
library's code object (no GPU needed): exactly one kernel, no spilled register, no scratch, 0 bytes of LDS (a wave per view: the reduction
is shuffles, nothing is shared) and at most 64 vector registers (eight waves a SIMD), and the figures of its committed row in
profiles/meter_views_kernel_resources.txt.  No other library holds anything named level_views."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")
LISTING = os.path.join(ROOT, "profiles", "meter_views_kernel_resources.txt")


def _kr():
    import kernel_resources as KR

    if not os.path.exists(os.path.join(KR.LLVM_BIN, "llvm-objdump")):
        pytest.skip("no llvm-objdump / llvm-readelf under " + KR.LLVM_BIN)
    return KR


@pytest.fixture(scope="module")
def rows():
    KR = _kr()
    pkg.build_native()
    return KR.from_library(api.meter_library_path())


def test_the_companion_holds_exactly_one_kernel_within_its_budgets(rows):
    assert [r["name"].count("lc3_level_views_kernel") for r in rows] == [1], [r["name"] for r in rows]
    r = rows[0]
    assert r.get("vgpr_spill_count", 0) == 0, r
    assert r.get("sgpr_spill_count", 0) == 0, r
    assert r.get("private_segment_fixed_size", 0) == 0, r  # no scratch
    assert r["group_segment_fixed_size"] == 0, r           # no LDS
    assert r["vgpr_count"] <= 64, r["vgpr_count"]


def test_the_committed_listing_is_the_built_kernel(rows):
    """profiles/meter_views_kernel_resources.txt is this kernel's row: name, vector and scalar registers, LDS, scratch and spills"""
    with open(LISTING) as f:
        lines = [ln.split() for ln in f.read().splitlines() if "lc3_level_views_kernel" in ln]
    assert len(lines) == 1 and len(lines[0]) == 7
    r, row = rows[0], lines[0]
    assert row[0] == r["name"]
    assert [int(x) for x in row[1:]] == [r["vgpr_count"], r["sgpr_count"], r["group_segment_fixed_size"], r.get("private_segment_fixed_size", 0),
                                        r.get("vgpr_spill_count", 0), r.get("sgpr_spill_count", 0)]


def test_the_companion_holds_nothing_of_the_other_libraries(rows):
    with open(api.meter_library_path(), "rb") as f:
        blob = f.read()
    for name in (b"lc3_inspect_views_kernel", b"lc3_analyze_views_kernel", b"lc3_mix_views_kernel", b"lc3_rate_views_kernel", b"lc3_parse_kernel",
                 b"lc3_enc_front"):
        assert name not in blob, name


def test_no_other_library_holds_anything_named_level_views():
    KR = _kr()
    main = pkg.build_native()
    for path in (main, api.inspector_library_path(), api.analyzer_library_path(), api.mixer_library_path(), api.resampler_library_path()):
        assert not [r["name"] for r in KR.from_library(path) if "level_views" in r["name"]], path
        with open(path, "rb") as f:
            assert b"level_views" not in f.read(), path
