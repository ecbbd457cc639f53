"""The C ABI of the meter (lc3gpu_meter_create / _destroy / _reset / _reset_channels, lc3gpu_measure_mixed_views: the PCM levels and the
speech gate of a tick, in place): declared in include/lc3gpu.h with the 24-byte descriptor and the 32-byte record, exported by the built MAIN
library -- whose own device code stays what it was: the kernel lives in a fifth companion library that the main library links with an
$ORIGIN run path --, bound by the Python layer, the C++ facade and the Rust binding with the header's sizes and field offsets, stated in the
header with the formulas and the refusal table, and refusing on the host what needs no device.  No GPU needed."""
import ctypes
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")

SYMBOLS = ["lc3gpu_meter_create", "lc3gpu_meter_destroy", "lc3gpu_meter_reset", "lc3gpu_meter_reset_channels", "lc3gpu_measure_mixed_views"]
EINVAL, ECHANNEL, ENODEVICE = -1, -2, -6
C_SIZES = {"int": 4, "int32_t": 4, "uint32_t": 4, "int64_t": 8, "int16_t": 2, "uint16_t": 2, "uint8_t": 1}
RUST = {"int": "i32", "int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "int16_t": "i16", "uint16_t": "u16", "uint8_t": "u8"}
NUMPY = {"int": "<i4", "int32_t": "<i4", "uint32_t": "<u4", "int64_t": "<i8", "int16_t": "<i2", "uint16_t": "<u2", "uint8_t": "|u1"}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _header():
    return _read("include", "lc3gpu.h")


def _struct(text, name):
    """[(field, C type, offset)] and the size of a struct of the header, by the C rules: every field at its natural alignment"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    fields, off, align = [], 0, 1
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.split(" ", 1)
        for f in names.split(","):
            size = C_SIZES[ctype]
            off = (off + size - 1) // size * size
            fields.append((f.strip(), ctype, off))
            off += size
            align = max(align, size)
    return fields, (off + align - 1) // align * align


def test_the_five_symbols_and_the_two_structs_are_declared_exported_and_bound_in_all_four_bindings():
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
    assert "typedef struct lc3gpu_meter lc3gpu_meter;" in text
    # sizes and field offsets: the header against the ctypes mirror (numpy) and the generated Rust structs
    for cname, dtype, rname, size in (("lc3gpu_meter_desc", api.METER_DESC_DTYPE, "Lc3GpuMeterDesc", 24), ("lc3gpu_level", api.LEVEL_DTYPE, "Lc3GpuLevel", 32)):
        fields, total = _struct(text, cname)
        assert total == size == dtype.itemsize, cname
        assert "static_assert(sizeof(%s) == %d" % (cname, size) in text and "_Static_assert(sizeof(%s) == %d" % (cname, size) in text
        assert dtype.names == tuple(f for f, _, _ in fields), cname
        for f, ctype, off in fields:
            assert dtype.fields[f][1] == off and dtype.fields[f][0].str == NUMPY[ctype], (cname, f)
        body = re.search(r"pub struct %s \{(.*?)\}" % rname, rs, flags=re.S).group(1)
        assert [tuple(x.strip().rstrip(",").replace("pub ", "").split(": ")) for x in body.strip().splitlines()] == [(f, RUST[c]) for f, c, _ in fields], rname
        assert "#[repr(C)]" in rs[rs.index("pub struct %s {" % rname) - 80:rs.index("pub struct %s {" % rname)]
        assert "size_of::<%s>() == %d" % (rname, size) in rs
    assert [f for f, _, _ in _struct(text, "lc3gpu_level")[0]] == ["sum_sq", "env", "sum", "min", "max", "n_clipped", "n_cross", "hang", "active", "reserved0",
                                                                   "reserved1"]
    assert [o for _, _, o in _struct(text, "lc3gpu_level")[0]] == [0, 8, 12, 16, 18, 20, 22, 24, 26, 27, 28]
    for method in ("measure_mixed_views", "reset", "reset_channels", "close"):
        assert hasattr(api.Lc3Meter, method), method
    assert pkg.Lc3Meter is api.Lc3Meter and pkg.METER_DESC_DTYPE is api.METER_DESC_DTYPE and pkg.LEVEL_DTYPE is api.LEVEL_DTYPE
    assert pkg.meter_library_path is api.meter_library_path and pkg.meter_plan_info is api.meter_plan_info
    assert "class Lc3Meter" in hpp and "pub struct Lc3MeterGpu" in rs and "measure_mixed_views_device" in rs and "pub struct Lc3GpuMeter {" in rs
    assert re.search(r"lc3gpu_meter_create\(lc3gpu_meter \*\*out, int n_channels, const lc3gpu_meter_desc \*descs, int max_views\)", text)
    assert re.search(r"lc3gpu_meter_reset_channels\(lc3gpu_meter \*mt, const int32_t \*channels, int n\)", text)
    assert re.search(r"lc3gpu_measure_mixed_views\(lc3gpu_meter \*mt, const lc3gpu_view \*views, int n_views, const int16_t \*d_pcm, size_t pcm_elems,\s*"
                     r"uint8_t \*d_active, size_t n_active,\s*lc3gpu_level \*d_levels, size_t n_levels,\s*void \*hip_stream\)", text)
    # behind the resampler's block
    assert _header().index("int lc3gpu_resample_mixed_views(") < _header().index("PCM levels over a list of VIEWS")
    # the ctypes signature: ten arguments, the three extents as size_t
    args = L.lc3gpu_measure_mixed_views.argtypes
    assert len(args) == 10 and [k for k, a in enumerate(args) if a is ctypes.c_size_t] == [4, 6, 8]


def test_the_fifth_companion_library_is_built_and_the_main_library_links_it():
    main = pkg.build_native()
    comp = api.meter_library_path()
    assert os.path.basename(comp) == "liblc3gpu_meter.so" and os.path.dirname(comp) == os.path.dirname(main)
    assert os.path.exists(comp) and os.path.exists(comp + ".stamp")
    out = subprocess.check_output(["ldd", main], text=True)
    line = [ln for ln in out.splitlines() if "liblc3gpu_meter.so" in ln]
    assert len(line) == 1 and "not found" not in line[0], out
    assert os.path.realpath(line[0].split("=>")[1].split("(")[0].strip()) == os.path.realpath(comp)  # (found through $ORIGIN: beside the main library)
    # the companion needs neither the main library nor the other four, and holds the host side under names of its own
    needs = subprocess.check_output(["ldd", comp], text=True)
    for other in ("liblc3gpu.so", "liblc3gpu_inspector", "liblc3gpu_analyzer", "liblc3gpu_mixer", "liblc3gpu_resampler"):
        assert other not in needs, other
    C = ctypes.CDLL(comp)
    for name in ("lc3mtr_create", "lc3mtr_destroy", "lc3mtr_reset", "lc3mtr_reset_channels", "lc3mtr_mixed_views", "lc3mtr_plan_info"):
        assert hasattr(C, name), name
    for name in SYMBOLS:
        assert not hasattr(C, name), name
    # the sources: a host-only unit in the main library, the device code in a unit of its own, the check in a header shared with the tests
    assert any(p.endswith("lc3gpu_meter_api.cpp") for p in api._HOST_SRCS)
    assert "__global__" not in _read("lc3-codec_amd", "csrc", "lc3gpu_meter_api.cpp")
    csrc = os.path.join(ROOT, "lc3-codec_amd", "csrc")
    for other in sorted(os.listdir(csrc)):  # the companion's sources are seen by its own unit only
        if other in api.companion_own("meter") or other == "lc3gpu_meter_api.cpp" or not other.endswith((".h", ".hip", ".cpp")):
            continue
        src = _read("lc3-codec_amd", "csrc", other)
        assert "measure_mixed_views" not in src and "lc3mtr_" not in src and "lc3_dev_level" not in src and "lc3_host_measure_views" not in src, other
        assert "level_views" not in src and "lc3_mt_" not in src and "lc3_lvl_" not in src, other
    hip = _read("lc3-codec_amd", "csrc", "lc3gpu_meter.hip")
    assert '#include "lc3_dev_level.h"' in hip and hip.count("__global__") == 1 and "lc3_level_views_kernel" in hip
    for piece in ("lc3_lvl_lane(", "lc3_lvl_combine(", "lc3_lvl_finish("):
        assert piece in hip, piece
    assert "__shared__" not in hip and "__syncthreads" not in hip  # no LDS, no barrier
    assert '#include "lc3_host_measure_views.h"' in _read("lc3-codec_amd", "csrc", "lc3_dev_level.h")
    host = _read("lc3-codec_amd", "csrc", "lc3_host_measure_views.h")
    assert '#include "lc3_host_inspect_views.h"' in host and "lc3_iv_inside(" in host and "lc3_iv_ranges_overlap(" in host and "hip_runtime" not in host
    for user in ("lc3_emu_meter_views.cpp", "lc3_meter_views_check_main.cpp"):
        assert '#include "../../lc3-codec_amd/csrc/lc3_dev_level.h"' in _read("tests", "emu", user), user
    # the meter's own sources are no part of what the other units are stamped with
    own = set(api.companion_own("meter"))
    assert own == {"lc3gpu_meter.hip", "lc3_host_measure_views.h", "lc3_dev_level.h"}
    names = lambda paths: {os.path.basename(p) for p in paths}
    assert own <= names(api.companion_sources("meter"))
    others = [c for c in api._COMPANIONS if c != "meter"]
    assert sorted(others) == ["analyzer", "inspector", "mixer", "resampler"]
    for other in others:  # hidden from the four other companions and from the main units
        assert not own & names(api.companion_sources(other)), other
    assert not own & names(api.main_sources())
    # the plan's figures, from the companion itself
    assert api.meter_plan_info() == (4, 256, 8, 16)


def test_the_header_states_the_contract_the_formulas_and_the_refusal_table():
    text = " ".join(re.sub(r"\n \*(?= )", " ", _header()).split())  # (a comment's lines joined: no " * " inside a sentence)
    m = re.search(r"PCM levels over a list of VIEWS(.*?)typedef struct lc3gpu_meter_desc", text)
    assert m, "the contract of the meter"
    c = m.group(1)
    for what in ("lc3gpu_mix_mixed_views", "lc3gpu_analyze_mixed_views", "does not depend on the order of summation", "one of the six rates", "7500 or 10000",
                 "0..32768", "0..2^30", "0..65535", "n_channels >= 1", "max_views >= 1 bounds n_views", "checked before a device is looked for",
                 "bound to the device that is current at creation", "not thread-safe", "independent of every other object", "LC3GPU_ENODEVICE", "HOST array",
                 "NOT read: nbytes, byte_off, byte_pitch", "the very array the tick gave lc3gpu_decode_mixed_views", "lc3gpu_encode_mixed_views",
                 "a channel may be named once per call: twice is LC3GPU_ECHANNEL", "d_pcm[pcm_off + t * pitch + n * pcm_stride]",
                 "d_levels[flag_off + t * fp]", "fp = flag_pitch ? flag_pitch : 1", "At least one output must be given", "left as it was",
                 "the last sample of frame t - 1 of the view", "ms = sum_sq / nf", "d = ms - env0; k = d > 0 ? attack_q15 : release_q15",
                 "env = env0 + ((d * k + 16384) >> 15)", "if env >= threshold: hang = hang_frames, active = 1", "else if hang0 > 0: hang = hang0 - 1, active = 1",
                 "else: hang = 0, active = 0", "last = x[nf - 1]", "sum_sq <= 480 * 2^30 < 2^39", "|sum| <= 15 728 640", "|d * k| <= 2^45",
                 "between env0 and ms inclusive", "A coefficient of 32768 reaches ms exactly", "a coefficient of 0 never moves",
                 "split over calls and over views' n_frames in any way without changing one record", "last = 0, env = 0, hang = 0",
                 "a channel not listed keeps its state", "wait for nothing and launch nothing", "read a fresh state inside their next launch",
                 "launched nothing, written nothing, advanced no channel and consumed no pending reset",
                 # the refusal table
                 "channel outside [0, n_channels) LC3GPU_ECHANNEL", "a channel named twice in one call LC3GPU_ECHANNEL", "n_frames < 1 LC3GPU_ELENGTH",
                 "more than 2^31 - 1 samples in one view LC3GPU_ELENGTH", "[0, pcm_elems) LC3GPU_ELENGTH", "of a GIVEN output LC3GPU_ELENGTH",
                 "n_views > max_views LC3GPU_ELENGTH", "pcm_stride outside 1..8 LC3GPU_EINVAL", "a negative pcm_off or flag_off LC3GPU_EINVAL",
                 "a non-zero pitch below nf * pcm_stride LC3GPU_EINVAL", "flag_pitch < 0 LC3GPU_EINVAL", "reserved != 0 LC3GPU_EINVAL",
                 "or a base not 4-byte aligned LC3GPU_EINVAL", "pcm_stride >= 2 with a base not 2-byte aligned LC3GPU_EINVAL", "both outputs NULL LC3GPU_EINVAL",
                 "d_levels not 16-byte aligned LC3GPU_EINVAL", "the other output's LC3GPU_EINVAL", "a null mt", "n_views < 0 LC3GPU_EINVAL",
                 "n_views == 0 LC3GPU_OK (nothing launched)", "unsigned 64-bit arithmetic that cannot wrap", "LC3GPU_EHIP", "asynchronous on hip_stream",
                 "ordered behind it by an event wait", "more calls are in flight than the ring has slots", "ONE launch and ONE upload of O(views) bytes",
                 "one serial wave",
                 # out of scope
                 "NOT provided", "state blobs", "a channel twice in a call", "float or wider PCM", "K-weighting, LUFS", "per-sample envelopes",
                 "host-resident buffers", "the pipeline object", "uniform handles"):
        assert what in c, what
    design = " ".join(_read("DESIGN.md").split())
    for what in ("PCM levels for a tick, in place", "lc3gpu_measure_mixed_views", "liblc3gpu_meter.so", "lc3_mviews_check", "lc3_level_views_kernel",
                 "one state buffer per channel", "profiles/meter_views_kernel_resources.txt", "profiles/meter_views_measurements.jsonl"):
        assert what in design, what
    assert "lc3gpu_measure_mixed_views" in " ".join(_read("INTEGRATION.md").split()) and "measure_mixed_views" in _read("README.md")


def test_the_argument_errors_that_need_no_device():
    pkg.build_native()
    L = pkg.load_library()
    h = ctypes.c_void_p()

    def descs(*rows):
        a = api.np.zeros(len(rows), api.METER_DESC_DTYPE)
        for k, r in enumerate(rows):
            a[k] = r
        return a

    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ok = (48000, 10000, 16384, 2048, 1 << 16, 2)
    good = descs(ok, (8000, 7500, 0, 32768, 1 << 30, 65535))
    create = lambda d, n, mv: L.lc3gpu_meter_create(ctypes.byref(h), n, None if d is None else P(d), mv)
    assert create(good, 2, 0) == EINVAL and create(good, 2, -1) == EINVAL and create(good, 0, 8) == EINVAL and create(None, 2, 8) == EINVAL
    assert L.lc3gpu_meter_create(None, 2, P(good), 8) == EINVAL
    # the descriptor checks run before the device is looked for
    for bad in ((22050, 10000) + ok[2:], (48000, 5000) + ok[2:], ok[:2] + (-1,) + ok[3:], ok[:2] + (32769,) + ok[3:], ok[:3] + (-1,) + ok[4:],
                ok[:3] + (32769,) + ok[4:], ok[:4] + ((1 << 30) + 1,) + ok[5:], ok[:5] + (-1,), ok[:5] + (65536,)):
        assert create(descs(ok, bad), 2, 8) == EINVAL, bad
    assert h.value is None
    views = api._view_list([(0, 2, 0, 1, 0, 0, 0)])
    dev = ctypes.c_void_p(256)  # never dereferenced: the meter is checked first
    assert L.lc3gpu_measure_mixed_views(None, P(views), 1, dev, 4096, ctypes.c_void_p(1 << 20), 4096, None, 0, None) == EINVAL
    assert L.lc3gpu_meter_destroy(None) == EINVAL and L.lc3gpu_meter_reset(None) == EINVAL
    assert L.lc3gpu_meter_reset_channels(None, None, 0) == EINVAL
    if pkg.device_count() == 0:  # no GPU here: creating a meter fails loudly
        assert create(good, 2, 8) == ENODEVICE and h.value is None
        try:
            api.Lc3Meter([ok], 4)
            assert False, "a meter without a device"
        except pkg.Lc3GpuError as e:
            assert e.code == ENODEVICE
