"""The C ABI of the mixer (lc3gpu_mixer_create / lc3gpu_mixer_destroy / lc3gpu_mix_mixed_views: the room mixes of a tick, in place):
declared in include/lc3gpu.h with the two 8-byte table entries, exported by the built MAIN library -- whose own device code stays what it
was: the kernel lives in a third companion library that the main library links with an $ORIGIN run path --, bound by the Python layer, the
C++ facade and the Rust binding, stated in the header with the formulas and the refusal table, and refusing on the host what needs no
device.  No GPU needed."""
import ctypes
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")

SYMBOLS = ["lc3gpu_mixer_create", "lc3gpu_mixer_destroy", "lc3gpu_mix_mixed_views"]
EINVAL, ELENGTH, ENODEVICE = -1, -3, -6


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _header():
    return _read("include", "lc3gpu.h")


def test_the_three_symbols_and_the_two_structs_are_declared_exported_and_bound_in_all_four_bindings():
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
    assert "typedef struct lc3gpu_mixer lc3gpu_mixer;" in text
    # the two table entries: 8 bytes each, asserted in the header for C and C++, in the Rust binding and in the Python layer
    assert re.search(r"typedef struct lc3gpu_mix_in \{\s*int32_t bus;\s*int32_t gain_q14;\s*\} lc3gpu_mix_in;", text)
    assert re.search(r"typedef struct lc3gpu_mix_out \{\s*int32_t bus;\s*int32_t minus;\s*\} lc3gpu_mix_out;", text)
    for s in ("lc3gpu_mix_in", "lc3gpu_mix_out"):
        assert "static_assert(sizeof(%s) == 8" % s in text and "_Static_assert(sizeof(%s) == 8" % s in text
    assert "size_of::<Lc3GpuMixIn>() == 8" in rs and "size_of::<Lc3GpuMixOut>() == 8" in rs
    assert "pub bus: i32,\n    pub gain_q14: i32," in rs and "pub bus: i32,\n    pub minus: i32," in rs
    assert api.MIX_IN_DTYPE.itemsize == 8 and api.MIX_OUT_DTYPE.itemsize == 8
    assert api.MIX_IN_DTYPE.names == ("bus", "gain_q14") and api.MIX_OUT_DTYPE.names == ("bus", "minus") and api.MIX_UNITY == 16384
    assert hasattr(api.Lc3Mixer, "mix_mixed_views") and pkg.Lc3Mixer is api.Lc3Mixer
    assert pkg.mixer_library_path is api.mixer_library_path and pkg.mixer_plan_info is api.mixer_plan_info
    assert "class Lc3Mixer" in hpp and "pub struct Lc3MixerGpu" in rs and "mix_mixed_views_device" in rs and "pub struct Lc3GpuMixer" in rs
    assert re.search(r"lc3gpu_mixer_create\(lc3gpu_mixer \*\*out, int n_streams, const lc3gpu_stream_desc \*descs, int max_views\)", text)
    assert re.search(r"lc3gpu_mix_mixed_views\(lc3gpu_mixer \*mx, const lc3gpu_view \*in_views, const lc3gpu_mix_in \*ins, int n_in, "
                     r"const int16_t \*d_pcm_in,\s*size_t in_elems, const lc3gpu_view \*out_views, const lc3gpu_mix_out \*outs, int n_out, "
                     r"int16_t \*d_pcm_out,\s*size_t out_elems, void \*hip_stream\)", text)


def test_the_third_companion_library_is_built_and_the_main_library_links_it():
    main = pkg.build_native()
    comp = api.mixer_library_path()
    assert os.path.basename(comp) == "liblc3gpu_mixer.so" and os.path.dirname(comp) == os.path.dirname(main)
    assert os.path.exists(comp) and os.path.exists(comp + ".stamp")
    out = subprocess.check_output(["ldd", main], text=True)
    line = [ln for ln in out.splitlines() if "liblc3gpu_mixer.so" in ln]
    assert len(line) == 1 and "not found" not in line[0], out
    assert os.path.realpath(line[0].split("=>")[1].split("(")[0].strip()) == os.path.realpath(comp)  # (found through $ORIGIN: beside the main library)
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", subprocess.check_output(["readelf", "-d", main], text=True))
    # the companion needs neither the main library nor the other two, and holds the host side under names of its own
    needs = subprocess.check_output(["ldd", comp], text=True)
    assert "liblc3gpu.so" not in needs and "liblc3gpu_inspector" not in needs and "liblc3gpu_analyzer" not in needs
    C = ctypes.CDLL(comp)
    for name in ("lc3mix_create", "lc3mix_destroy", "lc3mix_mixed_views", "lc3mix_plan_info"):
        assert hasattr(C, name), name
    for name in SYMBOLS:
        assert not hasattr(C, name), name
    # the sources: a host-only unit in the main library, the device code in a unit of its own, the check in a header shared with the tests
    assert any(p.endswith("lc3gpu_mixer_api.cpp") for p in api._HOST_SRCS)
    assert "__global__" not in _read("lc3-codec_amd", "csrc", "lc3gpu_mixer_api.cpp")
    for other in ("lc3gpu.hip", "lc3gpu_inspector.hip", "lc3gpu_analyzer.hip", "lc3_host_inspect_views.h", "lc3_host_analyze_views.h"):
        src = _read("lc3-codec_amd", "csrc", other)
        assert "mix_mixed_views" not in src and "mixer" not in src and "lc3_dev_mix" not in src and "lc3_host_mix_views" not in src, other
    hip = _read("lc3-codec_amd", "csrc", "lc3gpu_mixer.hip")
    assert '#include "lc3_dev_mix.h"' in hip and "lc3_mix_bus_pair(" in hip and hip.count("__global__") == 1 and "__syncthreads" not in hip
    assert '#include "lc3_host_mix_views.h"' in _read("lc3-codec_amd", "csrc", "lc3_dev_mix.h")
    host = _read("lc3-codec_amd", "csrc", "lc3_host_mix_views.h")
    assert '#include "lc3_host_inspect_views.h"' in host and "lc3_iv_inside(" in host and "lc3_iv_ranges_overlap(" in host and "hip_runtime" not in host
    for user in ("lc3_emu_mix_views.cpp", "lc3_mix_views_check_main.cpp"):
        assert '#include "../../lc3-codec_amd/csrc/lc3_dev_mix.h"' in _read("tests", "emu", user), user
    # the mixer's own sources are no part of what the other units are stamped with
    own = set(api.companion_own("mixer"))
    assert own == {"lc3gpu_mixer.hip", "lc3_host_mix_views.h", "lc3_dev_mix.h"}
    names = lambda paths: {os.path.basename(p) for p in paths}
    assert own <= names(api.companion_sources("mixer"))
    for other in api._COMPANIONS:
        assert other == "mixer" or not own & names(api.companion_sources(other)), other
    assert not own & names(api.main_sources())
    # the plan's figures, from the companion itself
    assert api.mixer_plan_info() == (512, 256, 8)


def test_the_header_states_the_contract_the_formulas_and_the_refusal_table():
    text = " ".join(re.sub(r"\n \*(?= )", " ", _header()).split())  # (a comment's lines joined: no " * " inside a sentence)
    m = re.search(r"Room mixes over two lists of VIEWS(.*?)typedef struct lc3gpu_mixer lc3gpu_mixer;", text)
    assert m, "the contract of the mixer"
    c = m.group(1)
    for what in ("lc3gpu_decode_mixed_views", "lc3gpu_encode_mixed_views", "no gather or scatter pass runs around the call", "The reference has no mixer",
                 "decoder/output_scaling.rs:24", "does not depend on the order of summation", "exactly as by lc3gpu_inspector_create", "8 kHz included",
                 "7500 or 10000", "1..400", "Only fs_hz and frame_us are used afterwards", "max_views >= 1 bounds n_in + n_out",
                 "bound to the device that is current at creation", "not thread-safe", "independent of every codec handle, of the inspector and of the analyzer",
                 "LC3GPU_ENODEVICE", "HOST arrays", "NOT read: nbytes, byte_off, byte_pitch, flag_off, flag_pitch", "ins[i] belongs to in_views[i]",
                 "one stream can feed two rooms", "unspecified", "inside the checked extents", "0 <= bus < max_views", "S = n_frames * nf",
                 "four 7.5 ms frames and three 10 ms frames mix", "44.1 kHz and 48 kHz", "d[pcm_off + (s / nf) * pitch + (s % nf) * pcm_stride]",
                 "term(i, s) = ((int32)in(i, s) * gain_q14[i] + 8192) >> 14", "ties upward", "0 for a bus without inputs",
                 "clamp(total(b, s) - (minus[o] >= 0 ? term(minus[o], s) : 0), -32768, 32767)", "gain_q14 = 16384 is unity", "N-1 mix", "left as it was",
                 "|term| <= 65536", "at most 16384 inputs", "|total| <= 2^30", "cannot leave int32",
                 # the refusal table
                 "launched nothing and written nothing", "channel outside [0, n_streams) LC3GPU_ECHANNEL", "n_frames < 1 LC3GPU_ELENGTH",
                 "more than 2^31 - 1 samples in one view LC3GPU_ELENGTH", "[0, out_elems) LC3GPU_ELENGTH", "n_in + n_out > max_views LC3GPU_ELENGTH",
                 "more than 16384 inputs on one bus LC3GPU_ELENGTH", "views of one bus with different S LC3GPU_ELENGTH",
                 "views of one bus with different fs_hz LC3GPU_EINVAL", "bus outside [0, max_views) LC3GPU_EINVAL",
                 "gain_q14 outside -32768..32767 LC3GPU_EINVAL", "naming an input of another bus LC3GPU_EINVAL", "pcm_stride outside 1..8 LC3GPU_EINVAL",
                 "a negative pcm_off LC3GPU_EINVAL", "a non-zero pitch below nf * pcm_stride LC3GPU_EINVAL", "reserved != 0 LC3GPU_EINVAL",
                 "or a base not 4-byte aligned LC3GPU_EINVAL", "pcm_stride >= 2 with a base not 2-byte aligned LC3GPU_EINVAL",
                 "+ 2 * out_elems) overlapping LC3GPU_EINVAL", "a null mx", "negative counts LC3GPU_EINVAL", "n_out == 0 LC3GPU_OK (nothing launched)",
                 "n_in == 0 with outputs LC3GPU_OK (the outputs are zeros)", "unsigned 64-bit arithmetic that cannot wrap",
                 "a workgroup must never overwrite what another still reads", "LC3GPU_EHIP", "asynchronous on hip_stream",
                 "more calls are in flight than the ring has slots", "ONE launch and ONE upload of O(views) bytes",
                 # out of scope
                 "NOT provided", "resampling between rates", "a gain per output", "ramps across a tick", "float or wider PCM", "host-resident buffers",
                 "the pipeline object", "uniform handles"):
        assert what in c, what
    design = " ".join(_read("DESIGN.md").split())
    for what in ("Room mixes for a tick, in place", "lc3gpu_mix_mixed_views", "liblc3gpu_mixer.so", "lc3_mviews_check", "lc3_mix_views_kernel", "lc3_mix_pair",
                 "profiles/mix_views_measurements.jsonl"):
        assert what in design, what
    assert "lc3gpu_mix_mixed_views" in " ".join(_read("INTEGRATION.md").split()) and "mix_mixed_views" in _read("README.md")


def test_the_argument_errors_that_need_no_device():
    pkg.build_native()
    L = pkg.load_library()
    h = ctypes.c_void_p()
    descs = api._desc_array([(48000, 10000, 40), (8000, 7500, 20)])
    create = lambda d, n, mv, out=h: L.lc3gpu_mixer_create(ctypes.byref(out) if out is not None else None, n, d, mv)
    assert create(descs, 2, 0) == EINVAL and create(descs, 2, -1) == EINVAL and create(descs, 0, 8) == EINVAL and create(None, 2, 8) == EINVAL
    assert L.lc3gpu_mixer_create(None, 2, descs, 8) == EINVAL
    assert create(api._desc_array([(48000, 5000, 40)]), 1, 8) == EINVAL and create(api._desc_array([(22050, 10000, 40)]), 1, 8) == EINVAL
    assert create(api._desc_array([(48000, 10000, 0)]), 1, 8) == ELENGTH and create(api._desc_array([(48000, 10000, 401)]), 1, 8) == ELENGTH
    assert h.value is None
    views = api._view_list([(0, 2, 0, 1, 0, 0, 0)])
    dev = ctypes.c_void_p(256)  # never dereferenced: the mixer is checked first
    pv = views.ctypes.data_as(ctypes.c_void_p)
    tab = api._mix_table([(0, 16384)], api.MIX_IN_DTYPE)
    assert L.lc3gpu_mix_mixed_views(None, pv, tab.ctypes.data_as(ctypes.c_void_p), 1, dev, 4096, pv, tab.ctypes.data_as(ctypes.c_void_p), 1,
                                    ctypes.c_void_p(1 << 20), 4096, None) == EINVAL
    assert L.lc3gpu_mixer_destroy(None) == EINVAL
    if pkg.device_count() == 0:  # no GPU here: creating a mixer fails loudly
        assert create(descs, 2, 8) == ENODEVICE and h.value is None
        try:
            api.Lc3Mixer([(48000, 10000, 40)], 4)
            assert False, "a mixer without a device"
        except pkg.Lc3GpuError as e:
            assert e.code == ENODEVICE
