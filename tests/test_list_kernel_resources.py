"""The wave-per-stream kernels of the list calls (lc3gpu_encode_list / lc3gpu_decode_list) against their uniform twins, read from the BUILT
library's code objects (no GPU needed).  Headline view (48 kHz / 10 ms): no spilled vector register, no more scratch and the same LDS as
the twin; the analysis halves within the 120 vector registers tests/test_kernel_resources.py allows the uniform ones; the synthesis kernels
within 128 -- their twins' own count (lc3_decode_kernel and lc3_decode_late_kernel both sit at 128, four waves per SIMD), which is also
what the list kernels were found at: the channel lookup and the per-stream flag live in scalar registers."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("lc3-codec_amd")

# list kernel (48 kHz / 10 ms view) -> (its uniform twin, most vector registers)
TWINS = {
    "lc3_enc_front_list_kernelI13lc3_cfg_48k10E": ("lc3_enc_front_kernelI13lc3_cfg_48k10E", 120),
    "lc3_enc_back_list_kernelI13lc3_cfg_48k10E": ("lc3_enc_back_kernelI13lc3_cfg_48k10E", 120),
    "lc3_decode_list_kernelI13lc3_cfg_48k10Li0E": ("lc3_decode_kernelI13lc3_cfg_48k10E", 128),
    "lc3_decode_list_kernelI13lc3_cfg_48k10Li1E": ("lc3_decode_late_kernelI13lc3_cfg_48k10E", 128),
}
# the run-time view serves every other configuration
RUNTIME_VIEW = ["lc3_enc_front_list_kernelI11lc3_cfg_anyE", "lc3_enc_back_list_kernelI11lc3_cfg_anyE", "lc3_decode_list_kernelI11lc3_cfg_anyLi0E",
                "lc3_decode_list_kernelI11lc3_cfg_anyLi1E"]


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


def test_list_headline_kernels_keep_their_twins_budgets(rows):
    for frag, (twin_frag, most) in TWINS.items():
        r, twin = _one(rows, frag), _one(rows, twin_frag)
        assert r.get("vgpr_spill_count", 0) == 0, (r["name"], r["vgpr_spill_count"])
        assert r["vgpr_count"] <= most, (r["name"], r["vgpr_count"], most)
        assert r["vgpr_count"] <= max(most, twin["vgpr_count"]), (r["name"], r["vgpr_count"], twin["vgpr_count"])
        assert r.get("private_segment_fixed_size", 0) <= twin.get("private_segment_fixed_size", 0), (r["name"], "scratch")
        assert r["group_segment_fixed_size"] == twin["group_segment_fixed_size"], (r["name"], "LDS")
        assert 4 * r["group_segment_fixed_size"] <= 160 * 1024, (r["name"], "four workgroups per compute unit")


def test_list_kernels_exist_for_the_run_time_view_with_the_twins_lds(rows):
    lds = {"front": _one(rows, "lc3_enc_front_kernelI11lc3_cfg_anyE")["group_segment_fixed_size"],
           "back": _one(rows, "lc3_enc_back_kernelI11lc3_cfg_anyE")["group_segment_fixed_size"],
           "decode": _one(rows, "lc3_decode_kernelI11lc3_cfg_anyE")["group_segment_fixed_size"]}
    for frag in RUNTIME_VIEW:
        r = _one(rows, frag)
        kind = "front" if "front" in frag else ("back" if "back" in frag else "decode")
        assert r["group_segment_fixed_size"] == lds[kind], (r["name"], "LDS")
