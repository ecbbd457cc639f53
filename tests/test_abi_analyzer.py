"""The C ABI of the analyzer (lc3gpu_analyzer_create / lc3gpu_analyzer_destroy / lc3gpu_analyze_mixed_views: frame spectra and band
energies for a tick, in place): declared in include/lc3gpu.h with LC3GPU_BANDS and LC3GPU_SPEC_LINES, exported by the built MAIN library --
whose own device code stays what it was: the kernel lives in a second companion library that the main library links with an $ORIGIN run
path --, bound by the Python layer, the C++ facade and the Rust binding, stated in the header with the refusal table and the equivalence,
and refusing on the host what needs no device.  No GPU needed."""
import ctypes
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")

SYMBOLS = ["lc3gpu_analyzer_create", "lc3gpu_analyzer_destroy", "lc3gpu_analyze_mixed_views"]
EINVAL, ELENGTH, ENODEVICE = -1, -3, -6


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _header():
    return _read("include", "lc3gpu.h")


def test_the_three_symbols_and_the_two_row_lengths_are_declared_exported_and_bound_in_all_four_bindings():
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
    assert "typedef struct lc3gpu_analyzer lc3gpu_analyzer;" in text
    assert re.search(r"^#define LC3GPU_BANDS 64\s*$", text, re.M) and re.search(r"^#define LC3GPU_SPEC_LINES 400\s*$", text, re.M)
    assert "LC3GPU_BANDS: i32 = 64" in rs and "LC3GPU_SPEC_LINES: i32 = 400" in rs
    assert (api.BANDS, api.SPEC_LINES) == (64, 400) and (pkg.BANDS, pkg.SPEC_LINES) == (64, 400)
    assert hasattr(api.Lc3Analyzer, "analyze_mixed_views") and pkg.Lc3Analyzer is api.Lc3Analyzer
    assert pkg.analyzer_library_path is api.analyzer_library_path and pkg.analyzer_plan_info is api.analyzer_plan_info
    assert "class Lc3Analyzer" in hpp and "pub struct Lc3AnalyzerGpu" in rs and "analyze_mixed_views_device" in rs
    assert "pub struct Lc3GpuAnalyzer" in rs
    # the extents travel with the arrays, in the header's order
    assert re.search(r"lc3gpu_analyzer_create\(lc3gpu_analyzer \*\*out, int n_streams, const lc3gpu_stream_desc \*descs, int max_views, "
                     r"int max_frames\)", text)
    assert re.search(r"lc3gpu_analyze_mixed_views\(lc3gpu_analyzer \*an, const lc3gpu_view \*views, int n_views, const uint8_t \*d_in, "
                     r"size_t in_bytes,\s*const uint8_t \*d_bad_frame, size_t n_flags,\s*float \*d_energy, size_t n_energy,\s*"
                     r"float \*d_bands, size_t n_bands,\s*float \*d_spec, size_t n_spec,\s*void \*hip_stream\)", text)


def test_the_second_companion_library_is_built_and_the_main_library_links_it():
    main = pkg.build_native()
    comp = api.analyzer_library_path()
    assert os.path.basename(comp) == "liblc3gpu_analyzer.so" and os.path.dirname(comp) == os.path.dirname(main)
    assert os.path.exists(comp) and os.path.exists(comp + ".stamp")
    out = subprocess.check_output(["ldd", main], text=True)
    line = [ln for ln in out.splitlines() if "liblc3gpu_analyzer.so" in ln]
    assert len(line) == 1 and "not found" not in line[0], out
    assert os.path.realpath(line[0].split("=>")[1].split("(")[0].strip()) == os.path.realpath(comp)  # (found through $ORIGIN: beside the main library)
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", subprocess.check_output(["readelf", "-d", main], text=True))
    # the companion needs neither the main library nor the inspector's, and holds the host side under names of its own
    needs = subprocess.check_output(["ldd", comp], text=True)
    assert "liblc3gpu.so" not in needs and "liblc3gpu_inspector" not in needs
    C = ctypes.CDLL(comp)
    for name in ("lc3ana_create", "lc3ana_destroy", "lc3ana_mixed_views", "lc3ana_plan_info"):
        assert hasattr(C, name), name
    for name in SYMBOLS:
        assert not hasattr(C, name), name
    # the sources: a host-only unit in the main library, the device code in a unit of its own, the check in a header shared with the tests
    assert any(p.endswith("lc3gpu_analyzer_api.cpp") for p in api._HOST_SRCS)
    assert "__global__" not in _read("lc3-codec_amd", "csrc", "lc3gpu_analyzer_api.cpp")
    main_src = _read("lc3-codec_amd", "csrc", "lc3gpu.hip")
    assert "analyze_mixed_views" not in main_src and "analyzer" not in main_src
    assert "analy" not in _read("lc3-codec_amd", "csrc", "lc3gpu_inspector.hip")
    hip = _read("lc3-codec_amd", "csrc", "lc3gpu_analyzer.hip")
    assert '#include "lc3_dev_dec_analyze.h"' in hip and '#include "lc3_host_analyze_views.h"' in hip and "lc3_analyze_frame(" in hip
    assert hip.count("__syncthreads()") == 1 and hip.count("__global__") == 1
    assert '#include "lc3_host_inspect_views.h"' in _read("lc3-codec_amd", "csrc", "lc3_host_analyze_views.h")
    assert '#include "../../lc3-codec_amd/csrc/lc3_host_analyze_views.h"' in _read("tests", "emu", "lc3_emu_analyze_views.cpp")
    # the analyzer's own sources are no part of what the other units are stamped with
    own = set(api.companion_own("analyzer"))
    assert own == {"lc3gpu_analyzer.hip", "lc3_host_analyze_views.h", "lc3_dev_dec_analyze.h"}
    names = lambda paths: {os.path.basename(p) for p in paths}
    assert own <= names(api.companion_sources("analyzer"))
    for other in api._COMPANIONS:
        assert other == "analyzer" or not own & names(api.companion_sources(other)), other
    assert not own & names(api.main_sources())
    # the plan's figures, from the companion itself
    assert api.analyzer_plan_info(40) == (256, 10672 + 256 * (72 + 40) + 8, 8, 648)
    assert api.analyzer_plan_info(400)[:2] == (64, 10672 + 64 * (72 + 400) + 8)


def test_the_header_states_the_contract_the_refusal_table_and_the_equivalence():
    text = " ".join(re.sub(r"\n \*(?= )", " ", _header()).split())  # (a comment's lines joined: no " * " inside a sentence)
    m = re.search(r"Frame analysis over a list of VIEWS(.*?)#define LC3GPU_BANDS", text)
    assert m, "the contract of the analyzer"
    c = m.group(1)
    for what in ("lc3gpu_decode_mixed_views and lc3gpu_inspect_mixed_views", "needs no codec handle", "ANALYZER", "exactly as for lc3gpu_inspector_create",
                 "8 kHz included", "7500 or 10000", "1..400", "max_views >= 1", "max_frames >= 1", "one column of 648 words per frame",
                 "bound to the device that is current at creation", "not thread-safe", "independent of every codec handle and of the inspector",
                 "LC3GPU_ENODEVICE", "HOST lc3gpu_view[n_views]", "NOT read: pcm_stride, pcm_off, pcm_pitch", "i = flag_off + t * flag_pitch",
                 "d_in[byte_off + t * byte_pitch", "d_bad_frame[i]", "d_energy[i]", "d_bands[i * LC3GPU_BANDS", "d_spec[i * LC3GPU_SPEC_LINES",
                 "a pitch of 0 stands for the compact one", "At least one of the three outputs", "left as it was", "MAY be named by several views",
                 "a ring that wraps", "unspecified", "inside the checked extents",
                 # what is written
                 "reports status 0", "x_hat after spectral_noise_shaping::decode", "0.0f for ne <= k < 400", "LC3GPU_DBG_SPEC dump of lc3gpu_decode_frame_debug",
                 "encoder/modified_dct.rs:140-152", "e += x[k] * x[k] / (float)(I[b + 1] - I[b])", "0.0f for nb <= b < 64", "multiply, then divide, then add",
                 "nothing fused", "d_energy[i] = -1.0f", "rows are all 0.0f", "does not conceal",
                 "d_energy[i] < 0 exactly where lc3gpu_inspect_mixed_views writes a non-zero status",
                 # the refusal table
                 "launched nothing and written nothing", "channel outside [0, n_streams) LC3GPU_ECHANNEL", "n_frames < 1 LC3GPU_ELENGTH",
                 "nbytes not 0 and outside 1..400 LC3GPU_ELENGTH", "more than 2^31 - 1 frames in one call LC3GPU_ELENGTH",
                 "more than max_frames frames in one call LC3GPU_ELENGTH", "n_views > max_views LC3GPU_ELENGTH",
                 "[0, n_energy), [0, n_bands), [0, n_spec) LC3GPU_ELENGTH", "a negative byte_off or flag_off LC3GPU_EINVAL",
                 "a non-zero pitch below its minimum (nb, 1) LC3GPU_EINVAL", "reserved != 0 LC3GPU_EINVAL", "all three outputs NULL LC3GPU_EINVAL",
                 "null an, views or d_in LC3GPU_EINVAL", "n_views < 0 LC3GPU_EINVAL", "d_energy or d_bands not 4-byte aligned LC3GPU_EINVAL",
                 "d_spec not 16-byte aligned LC3GPU_EINVAL", "or another output's LC3GPU_EINVAL", "n_views == 0 LC3GPU_OK (nothing launched)",
                 "unsigned 64-bit arithmetic that cannot wrap", "only against the arrays that are given", "LC3GPU_EHIP", "asynchronous on hip_stream",
                 "does not synchronise the host", "more calls are in flight than the ring has slots", "share its scratch columns", "an event wait",
                 "ONE launch and ONE upload",
                 # out of scope
                 "NOT provided", "a size per frame within a view", "uniform handles and flat batches", "PCM-domain measures", "concealed spectra",
                 "host-resident buffers", "pipeline object"):
        assert what in c, what
    design = " ".join(_read("DESIGN.md").split())
    for what in ("lc3gpu_analyze_mixed_views", "liblc3gpu_analyzer.so", "lc3_aviews_check", "lc3_analyze_views_kernel", "lc3_analyze_frame",
                 "profiles/analyze_views_measurements.jsonl"):
        assert what in design, what
    assert "lc3gpu_analyze_mixed_views" in " ".join(_read("INTEGRATION.md").split()) and "analyze_mixed_views" in _read("README.md")


def test_the_argument_errors_that_need_no_device():
    pkg.build_native()
    L = pkg.load_library()
    h = ctypes.c_void_p()
    descs = api._desc_array([(48000, 10000, 40), (8000, 7500, 20)])
    create = lambda d, n, mv, mf, out=h: L.lc3gpu_analyzer_create(ctypes.byref(out) if out is not None else None, n, d, mv, mf)
    assert create(descs, 2, 0, 8) == EINVAL and create(descs, 0, 8, 8) == EINVAL and create(None, 2, 8, 8) == EINVAL
    assert create(descs, 2, 8, 0) == EINVAL and create(descs, 2, 8, -1) == EINVAL
    assert L.lc3gpu_analyzer_create(None, 2, descs, 8, 8) == EINVAL
    assert create(api._desc_array([(48000, 5000, 40)]), 1, 8, 8) == EINVAL and create(api._desc_array([(22050, 10000, 40)]), 1, 8, 8) == EINVAL
    assert create(api._desc_array([(48000, 10000, 0)]), 1, 8, 8) == ELENGTH and create(api._desc_array([(48000, 10000, 401)]), 1, 8, 8) == ELENGTH
    assert h.value is None
    views = api._view_list([(0, 2, 0, 1, 0, 0, 0)])
    dev = ctypes.c_void_p(256)  # never dereferenced: the analyzer is checked first
    assert L.lc3gpu_analyze_mixed_views(None, views.ctypes.data_as(ctypes.c_void_p), 1, dev, 4096, None, 0, dev, 4096, None, 0, None, 0, None) == EINVAL
    assert L.lc3gpu_analyzer_destroy(None) == EINVAL
    if pkg.device_count() == 0:  # no GPU here: creating an analyzer fails loudly
        assert create(descs, 2, 8, 8) == ENODEVICE and h.value is None
        try:
            api.Lc3Analyzer([(48000, 10000, 40)], 4, 16)
            assert False, "an analyzer without a device"
        except pkg.Lc3GpuError as e:
            assert e.code == ENODEVICE
