"""The C ABI of the resampler (lc3gpu_resampler_create / _destroy / _reset / _reset_channels, lc3gpu_resample_mixed_views: the rate
conversions of a tick, in place): declared in include/lc3gpu.h with the 12-byte descriptor, exported by the built MAIN library -- whose own
device code stays what it was: the kernel lives in a fourth companion library that the main library links with an $ORIGIN run path --,
bound by the Python layer, the C++ facade and the Rust binding, stated in the header with the formulas and the refusal table, and refusing
on the host what needs no device.  No GPU needed."""
import ctypes
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")

SYMBOLS = ["lc3gpu_resampler_create", "lc3gpu_resampler_destroy", "lc3gpu_resampler_reset", "lc3gpu_resampler_reset_channels", "lc3gpu_resample_mixed_views"]
EINVAL, ECHANNEL, ENODEVICE, EUNSUPPORTED = -1, -2, -6, -7


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _header():
    return _read("include", "lc3gpu.h")


def test_the_five_symbols_and_the_descriptor_are_declared_exported_and_bound_in_all_four_bindings():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    pkg.build_native()
    L = pkg.load_library()
    hpp, rs = _read("include", "lc3gpu.hpp"), _read("bindings", "lc3gpu.rs")
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/lc3gpu.h"
        assert hasattr(L, name), name + " is not exported by the built library"
        assert name in api.ABI_SYMBOLS, name
        assert name in hpp, name + " has no facade method in include/lc3gpu.hpp"
        assert re.search(r"pub fn %s\(" % name, rs), name + " is not declared in bindings/lc3gpu.rs"
    assert "typedef struct lc3gpu_resampler lc3gpu_resampler;" in text
    assert re.search(r"typedef struct lc3gpu_rate_desc \{\s*int fs_in_hz;\s*int fs_out_hz;\s*int frame_us;\s*\} lc3gpu_rate_desc;", text)
    assert "static_assert(sizeof(lc3gpu_rate_desc) == 12" in text and "_Static_assert(sizeof(lc3gpu_rate_desc) == 12" in text
    assert "size_of::<Lc3GpuRateDesc>() == 12" in rs and "pub fs_in_hz: i32,\n    pub fs_out_hz: i32,\n    pub frame_us: i32," in rs
    assert api.RATE_DESC_DTYPE.itemsize == 12 and api.RATE_DESC_DTYPE.names == ("fs_in_hz", "fs_out_hz", "frame_us")
    for method in ("resample_mixed_views", "reset", "reset_channels"):
        assert hasattr(api.Lc3Resampler, method), method
    assert pkg.Lc3Resampler is api.Lc3Resampler and pkg.RATE_DESC_DTYPE is api.RATE_DESC_DTYPE
    assert pkg.resampler_library_path is api.resampler_library_path and pkg.resampler_plan_info is api.resampler_plan_info
    assert "class Lc3Resampler" in hpp and "pub struct Lc3ResamplerGpu" in rs and "resample_mixed_views_device" in rs and "pub struct Lc3GpuResampler" in rs
    assert re.search(r"lc3gpu_resampler_create\(lc3gpu_resampler \*\*out, int n_channels, const lc3gpu_rate_desc \*descs, int max_views\)", text)
    assert re.search(r"lc3gpu_resampler_reset_channels\(lc3gpu_resampler \*rs, const int32_t \*channels, int n\)", text)
    assert re.search(r"lc3gpu_resample_mixed_views\(lc3gpu_resampler \*rs, const lc3gpu_view \*in_views, const int16_t \*d_pcm_in, size_t in_elems,\s*"
                     r"const lc3gpu_view \*out_views, int16_t \*d_pcm_out, size_t out_elems, int n_views, void \*hip_stream\)", text)
    # behind the mixer's block
    assert _header().index("int lc3gpu_mix_mixed_views(") < _header().index("Rate conversion over two lists of VIEWS")


def test_the_fourth_companion_library_is_built_and_the_main_library_links_it():
    main = pkg.build_native()
    comp = api.resampler_library_path()
    assert os.path.basename(comp) == "liblc3gpu_resampler.so" and os.path.dirname(comp) == os.path.dirname(main)
    assert os.path.exists(comp) and os.path.exists(comp + ".stamp")
    out = subprocess.check_output(["ldd", main], text=True)
    line = [ln for ln in out.splitlines() if "liblc3gpu_resampler.so" in ln]
    assert len(line) == 1 and "not found" not in line[0], out
    assert os.path.realpath(line[0].split("=>")[1].split("(")[0].strip()) == os.path.realpath(comp)  # (found through $ORIGIN: beside the main library)
    # the companion needs neither the main library nor the other three, and holds the host side under names of its own
    needs = subprocess.check_output(["ldd", comp], text=True)
    assert "liblc3gpu.so" not in needs and "liblc3gpu_inspector" not in needs and "liblc3gpu_analyzer" not in needs and "liblc3gpu_mixer" not in needs
    C = ctypes.CDLL(comp)
    for name in ("lc3rs_create", "lc3rs_destroy", "lc3rs_reset", "lc3rs_reset_channels", "lc3rs_mixed_views", "lc3rs_plan_info"):
        assert hasattr(C, name), name
    for name in SYMBOLS:
        assert not hasattr(C, name), name
    # the sources: a host-only unit in the main library, the device code in a unit of its own, the check in a header shared with the tests
    assert any(p.endswith("lc3gpu_resampler_api.cpp") for p in api._HOST_SRCS)
    assert "__global__" not in _read("lc3-codec_amd", "csrc", "lc3gpu_resampler_api.cpp")
    for other in ("lc3gpu.hip", "lc3gpu_inspector.hip", "lc3gpu_analyzer.hip", "lc3gpu_mixer.hip", "lc3_host_inspect_views.h", "lc3_host_analyze_views.h",
                  "lc3_host_mix_views.h", "lc3_dev_mix.h"):
        src = _read("lc3-codec_amd", "csrc", other)
        # (the word "resampler" alone proves nothing: the main library's encoder has the LTPF resampler)
        assert "resample_mixed_views" not in src and "lc3rs_" not in src and "lc3_dev_resample" not in src and "lc3_host_resample_views" not in src, other
        assert "rate_views" not in src and "lc3_resample_tables" not in src, other
    hip = _read("lc3-codec_amd", "csrc", "lc3gpu_resampler.hip")
    assert '#include "lc3_dev_resample.h"' in hip and hip.count("__global__") == 1 and "lc3_rate_views_kernel" in hip
    for phase in ("lc3_rs_stage(", "lc3_rs_compute(", "lc3_rs_store("):
        assert phase in hip, phase
    assert '#include "lc3_host_resample_views.h"' in _read("lc3-codec_amd", "csrc", "lc3_dev_resample.h")
    host = _read("lc3-codec_amd", "csrc", "lc3_host_resample_views.h")
    assert '#include "lc3_host_inspect_views.h"' in host and "lc3_iv_inside(" in host and "lc3_iv_ranges_overlap(" in host and "hip_runtime" not in host
    assert '#include "../../tables/lc3_resample_tables.h"' in host
    for user in ("lc3_emu_resample_views.cpp", "lc3_resample_views_check_main.cpp"):
        assert '#include "../../lc3-codec_amd/csrc/lc3_dev_resample.h"' in _read("tests", "emu", user), user
    # the resampler's own sources are no part of what the other units are stamped with
    own = set(api.companion_own("resampler"))
    assert own == {"lc3gpu_resampler.hip", "lc3_host_resample_views.h", "lc3_dev_resample.h", "lc3_resample_tables.h"}
    names = lambda paths: {os.path.basename(p) for p in paths}
    assert own <= names(api.companion_sources("resampler"))
    for other in api._COMPANIONS:
        assert other == "resampler" or not own & names(api.companion_sources(other)), other
    assert not own & names(api.main_sources())
    # the plan's figures, from the companion itself
    assert api.resampler_plan_info() == (768, 256, 8, 96)


def test_the_header_states_the_contract_the_formulas_and_the_refusal_table():
    text = " ".join(re.sub(r"\n \*(?= )", " ", _header()).split())  # (a comment's lines joined: no " * " inside a sentence)
    m = re.search(r"Rate conversion over two lists of VIEWS(.*?)typedef struct lc3gpu_rate_desc", text)
    assert m, "the contract of the resampler"
    c = m.group(1)
    for what in ("lc3gpu_decode_mixed_views", "lc3gpu_mix_mixed_views", "lc3gpu_encode_mixed_views", "does not depend on the order of summation",
                 "tables/lc3_resample_tables.h", "7500 or 10000", "one of the six rates", "an exact copy: no delay, no state", "LC3GPU_EUNSUPPORTED",
                 "not 10 ms long", "n_channels >= 1", "max_views >= 1 bounds n_views", "bound to the device that is current at creation", "not thread-safe",
                 "independent of every codec handle, of the inspector, of the analyzer and of the mixer", "LC3GPU_ENODEVICE", "HOST arrays",
                 "in_views[i] and out_views[i] belong together", "NOT read: nbytes, byte_off, byte_pitch, flag_off, flag_pitch",
                 "the very array the tick gave lc3gpu_decode_mixed_views", "a channel may be named once per call: twice is LC3GPU_ECHANNEL",
                 "d[pcm_off + (s / nf) * pitch + (s % nf) * pcm_stride]", "nf = nf_in", "nf = nf_out", "L = fs_out_hz / g, M = fs_in_hz / g", "twelve ratios",
                 "S_out * M == S_in * L", "u = m * M; p = u % L; b = u / L", "c[p][j] * x[b - j]", "clamp((acc(m) + 16384) >> 15, -32768, 32767)",
                 "new history = the last T - 1 samples of (old history ++ x)", "left as it was", "always starts at phase 0",
                 "The group delay is 8 samples of the lower of the two rates", "sums to exactly 32768", "sum |c| <= 65535", "nothing wraps",
                 "Q = max(L, M), N = 16 Q + 1", "kaiser(N, beta = 6.0)", "fc = 0.92 * 0.5 / Q", "T = ceil(N / L)", "h[p + L j]",
                 "added to the phase's tap of largest magnitude", "COMMITTED table is the definition",
                 "a channel not listed keeps its history byte for byte", "wait for nothing and launch nothing", "read a zero history inside their next launch",
                 "launched nothing, written nothing, advanced no channel and consumed no pending reset",
                 # the refusal table
                 "channel outside [0, n_channels) LC3GPU_ECHANNEL", "a channel named twice in one call LC3GPU_ECHANNEL", "n_frames < 1 LC3GPU_ELENGTH",
                 "more than 2^31 - 1 samples in one view LC3GPU_ELENGTH", "[0, out_elems) LC3GPU_ELENGTH", "n_views > max_views LC3GPU_ELENGTH",
                 "more than 2^31 - 1 workgroups in the plan LC3GPU_ELENGTH", "channel or n_frames differing within a pair LC3GPU_EINVAL",
                 "pcm_stride outside 1..8 LC3GPU_EINVAL", "a negative pcm_off LC3GPU_EINVAL", "a non-zero pitch below nf * pcm_stride LC3GPU_EINVAL",
                 "reserved != 0 LC3GPU_EINVAL", "or a base not 4-byte aligned LC3GPU_EINVAL", "pcm_stride >= 2 with a base not 2-byte aligned LC3GPU_EINVAL",
                 "+ 2 * out_elems) overlapping LC3GPU_EINVAL", "a null rs", "n_views < 0 LC3GPU_EINVAL", "n_views == 0 LC3GPU_OK (nothing launched)",
                 "unsigned 64-bit arithmetic that cannot wrap", "LC3GPU_EHIP", "asynchronous on hip_stream", "ordered behind it by an event wait",
                 "more calls are in flight than the ring has slots", "ONE launch and ONE upload of O(views) bytes",
                 # out of scope
                 "NOT provided", "44.1 kHz conversion", "arbitrary ratios", "state blobs", "a channel twice in a call", "float or wider PCM",
                 "host-resident buffers", "the pipeline object", "uniform handles"):
        assert what in c, what
    design = " ".join(_read("DESIGN.md").split())
    for what in ("Rate conversion for a tick, in place", "lc3gpu_resample_mixed_views", "liblc3gpu_resampler.so", "lc3_rviews_check", "lc3_rate_views_kernel",
                 "two history buffers", "profiles/resample_views_kernel_resources.txt"):
        assert what in design, what
    assert "lc3gpu_resample_mixed_views" in " ".join(_read("INTEGRATION.md").split()) and "resample_mixed_views" in _read("README.md")


def test_the_argument_errors_that_need_no_device():
    pkg.build_native()
    L = pkg.load_library()
    h = ctypes.c_void_p()

    def descs(*rows):
        a = api.np.zeros(len(rows), api.RATE_DESC_DTYPE)
        for k, r in enumerate(rows):
            a[k] = r
        return a

    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = descs((16000, 48000, 10000), (48000, 8000, 7500))
    create = lambda d, n, mv: L.lc3gpu_resampler_create(ctypes.byref(h), n, None if d is None else P(d), mv)
    assert create(good, 2, 0) == EINVAL and create(good, 2, -1) == EINVAL and create(good, 0, 8) == EINVAL and create(None, 2, 8) == EINVAL
    assert L.lc3gpu_resampler_create(None, 2, P(good), 8) == EINVAL
    assert create(descs((48000, 48000, 5000)), 1, 8) == EINVAL and create(descs((22050, 48000, 10000)), 1, 8) == EINVAL
    assert create(descs((48000, 22050, 10000)), 1, 8) == EINVAL
    for fi, fo in ((44100, 48000), (48000, 44100), (8000, 44100)):
        assert create(descs((16000, 16000, 10000), (fi, fo, 10000)), 2, 8) == EUNSUPPORTED, (fi, fo)
    assert h.value is None
    views = api._view_list([(0, 2, 0, 1, 0, 0, 0)])
    dev = ctypes.c_void_p(256)  # never dereferenced: the resampler is checked first
    assert L.lc3gpu_resample_mixed_views(None, P(views), dev, 4096, P(views), ctypes.c_void_p(1 << 20), 4096, 1, None) == EINVAL
    assert L.lc3gpu_resampler_destroy(None) == EINVAL and L.lc3gpu_resampler_reset(None) == EINVAL
    assert L.lc3gpu_resampler_reset_channels(None, None, 0) == EINVAL
    if pkg.device_count() == 0:  # no GPU here: creating a resampler fails loudly
        assert create(good, 2, 8) == ENODEVICE and h.value is None
        assert create(descs((44100, 44100, 7500)), 1, 8) == ENODEVICE  # (a 44.1 kHz copy is a channel like any other)
        try:
            api.Lc3Resampler([(16000, 48000, 10000)], 4)
            assert False, "a resampler without a device"
        except pkg.Lc3GpuError as e:
            assert e.code == ENODEVICE
