"""CPU-side checks of the drop-in boundary: the C ABI library builds, loads and exports every symbol
include/lc3gpu.h declares; host logic that needs no GPU (config, working-buffer lengths, error strings)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")


@pytest.fixture(scope="module")
def L():
    pkg.build_native()
    return pkg.load_library()


def header_symbols():
    text = open(os.path.join(ROOT, "include", "lc3gpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lc3gpu_\w+)\s*\(", text)))


def test_library_exports_every_declared_symbol(L):
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(L, s), f"liblc3gpu.so does not export {s}"
    assert sorted(api.ABI_SYMBOLS) == syms


def test_rust_binding_binds_every_symbol_with_the_headers_parameter_lists():
    """bindings/lc3gpu.rs (shipped uncompiled: no Rust toolchain here) is what tools/gen_rust_binding.py writes from include/lc3gpu.h: the
    extern block names every declared symbol exactly once, with as many parameters as the header's declaration has"""
    import subprocess
    import sys
    import tempfile

    rs_path = os.path.join(ROOT, "bindings", "lc3gpu.rs")
    rs = open(rs_path).read()
    block = rs[rs.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    bound = re.findall(r"pub fn (lc3gpu_\w+)\((.*?)\)(?: -> [^;]+)?;", block)
    assert sorted(n for n, _ in bound) == header_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lc3gpu.h")).read(), flags=re.S)
    for name, params in bound:
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, text, flags=re.S)
        c_params = [q for q in " ".join(m.group(1).split()).split(",") if q.strip() and q.strip() != "void"]
        assert len([q for q in params.split(",") if q.strip()]) == len(c_params), name
    for code in ("LC3GPU_EPAIR: i32 = -8", "LC3GPU_EBITS: i32 = -4", "LC3GPU_LAYOUT_INTERLEAVED: i32 = 1"):
        assert code in rs
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "lc3gpu.rs")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_binding.py"), out])
        assert open(out).read() == rs, "bindings/lc3gpu.rs is stale: run tools/gen_rust_binding.py"


def test_signatures_are_plain_c():
    text = open(os.path.join(ROOT, "include", "lc3gpu.h")).read()
    assert "torch" not in text.lower().replace("no torch", "")
    assert "std::" not in text and "hipStream_t" not in text.replace("(a hipStream_t", "")


def test_config_matches_reference_table(L):  # common/config.rs:57-88, test :109-119
    c = pkg.Lc3Config(pkg.SamplingFrequency.Hz48000, pkg.FrameDuration.TenMs)
    assert (c.fs, c.fs_ind, c.z, c.nf, c.nb, c.ne) == (48000, 4, 180, 480, 64, 400)
    c = pkg.Lc3Config(8000, 7500)
    assert (c.nf, c.ne, c.nb, c.z) == (60, 60, 60, 14)
    c = pkg.Lc3Config(44100, 7500)
    assert (c.fs_ind, c.nf, c.ne) == (4, 360, 300)
    with pytest.raises(pkg.Lc3GpuError):
        pkg.Lc3Config(48000, 5000)


def test_working_buffer_lengths(L):  # lc3_encoder.rs:194-209, lc3_decoder.rs:236-244, README.md:130
    assert pkg.Lc3Encoder.calc_working_buffer_lengths(1, 10000, 48000) == (1900, 1106, 960)
    assert pkg.Lc3Encoder.calc_working_buffer_lengths(2, 10000, 48000) == (3800, 2212, 1920)
    assert pkg.Lc3Decoder.calc_working_buffer_lengths(1, 10000, 48000) == (4971, 960)
    import oracle_lib as O

    for fs in (8000, 16000, 24000, 32000, 44100, 48000):
        for us in (7500, 10000):
            e = np.zeros(3, np.int64)
            d = np.zeros(2, np.int64)
            O.lib().lc3o_encoder_working_buffer_lengths(3, fs, us, O.P(e))
            O.lib().lc3o_decoder_working_buffer_lengths(3, fs, us, O.P(d))
            assert pkg.Lc3Encoder.calc_working_buffer_lengths(3, us, fs) == tuple(e.tolist())
            assert pkg.Lc3Decoder.calc_working_buffer_lengths(3, us, fs) == tuple(d.tolist())


def test_error_strings_and_no_fallback(L):
    assert L.lc3gpu_strerror(0) == b"ok"
    assert b"16 bits" in L.lc3gpu_strerror(-4)
    assert b"pair" in L.lc3gpu_strerror(-8)
    assert L.lc3gpu_version() >= 100
    if pkg.device_count() == 0:
        # no GPU here: constructing a codec must fail loudly, never fall back to a CPU path
        with pytest.raises(pkg.Lc3EncoderError) as e:
            pkg.Lc3Encoder(1, 10000, 48000)
        assert e.value.code == -6
        with pytest.raises(pkg.Lc3DecoderError):
            pkg.Lc3Decoder(1, 10000, 48000)
        with pytest.raises(pkg.Lc3GpuError) as e:
            pkg.Lc3Pipeline(8, 10000, 48000)
        assert e.value.code == -6


def test_product_does_not_touch_the_oracle():
    """the shipped package must not import, link or execute anything under oracle/ or tests/"""
    pdir = os.path.join(ROOT, "lc3-codec_amd")
    for dirpath, _, files in os.walk(pdir):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in src.replace("CPU oracle", "").replace("the oracle", "").lower() or f == "synth.py", \
                    f"{f} mentions the oracle"
    out = os.popen(f"ldd {pkg.library_path()}").read()
    assert "oracle" not in out


def test_translation_units_match_the_generated_views():
    """the multi-unit build's list of units (api._translation_units) against lc3_cfg_views.h: the main unit, an encoder and a decoder unit
    for every view beyond the base ones, eight mixed-kernel units; the generated header is what tools/gen_views.py writes"""
    import re
    import subprocess
    import sys

    api = importlib.import_module("lc3-codec_amd.api")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = os.path.join(root, "lc3-codec_amd", "csrc", "lc3_cfg_views.h")
    text = open(hdr).read()
    n_all = int(re.search(r"#define LC3_N_VIEWS_ALL (\d+)", text).group(1))
    n_base = int(re.search(r"#define LC3_N_VIEWS_BASE (\d+)", text).group(1))
    assert (n_all, n_base) == (12, 4)  # 8 / 16 / 24 / 32 / 44.1 / 48 kHz x 7.5 / 10 ms; the whole-source build's four
    assert len(re.findall(r"^LC3_DEFINE_CFG_VIEW\(", text, re.M)) == n_all and len(re.findall(r"^LC3_DEFINE_FFT_PLAN\(", text, re.M)) == 9
    units = api._translation_units()
    assert units[0] == (0, 0) and len(units) == 1 + 2 * (n_all - n_base) + 8
    assert sorted(u[1] for u in units if u[0] == 1) == list(range(n_base + 1, n_all + 1)) == sorted(u[1] for u in units if u[0] == 3)
    assert sorted(u[1] for u in units if u[0] == 2) == list(range(8))
    # the header is reproducible from the generator
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "views.h")
        subprocess.check_call([sys.executable, os.path.join(root, "tools", "gen_views.py"), out])
        assert open(out, "rb").read() == open(hdr, "rb").read()


def test_the_pair_flag_peeks_are_carried_through_every_binding(L):
    """lc3gpu_{encoder,decoder}_pair_pending (what lets the pipeline refuse a submission before any group launches): header, library,
    Python binding, C++ facade, Rust binding; a null handle is refused, no device needed"""
    hpp = open(os.path.join(ROOT, "include", "lc3gpu.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "lc3gpu.rs")).read()
    for name in ("lc3gpu_encoder_pair_pending", "lc3gpu_decoder_pair_pending"):
        assert name in header_symbols() and name in api.ABI_SYMBOLS and name in hpp and "pub fn %s(" % name in rs
        assert getattr(L, name)(None) == -1  # LC3GPU_EINVAL
    assert hpp.count("bool pair_pending() const") == 2
    assert callable(pkg.Lc3Encoder.pair_pending) and callable(pkg.Lc3Decoder.pair_pending)
