"""The C ABI of the inspector (lc3gpu_inspector_create / lc3gpu_inspector_destroy / lc3gpu_inspect_mixed_views: frame status for a tick,
in place): declared in include/lc3gpu.h, exported by the built MAIN library -- whose own device code stays what it was: the kernel lives
in a companion library that the main library links with an $ORIGIN run path --, bound by the Python layer, the C++ facade and the Rust
binding, stated in the header with the refusal table and the two equivalences, and refusing on the host what needs no device.  No GPU
needed."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")

SYMBOLS = ["lc3gpu_inspector_create", "lc3gpu_inspector_destroy", "lc3gpu_inspect_mixed_views"]
EINVAL, ELENGTH, ENODEVICE = -1, -3, -6


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _header():
    return _read("include", "lc3gpu.h")


def test_the_three_symbols_are_declared_exported_and_bound_in_all_four_bindings():
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
    assert "typedef struct lc3gpu_inspector lc3gpu_inspector;" in text
    assert hasattr(api.Lc3Inspector, "inspect_mixed_views") and pkg.Lc3Inspector is api.Lc3Inspector
    assert "class Lc3Inspector" in hpp and "pub struct Lc3InspectorGpu" in rs and "inspect_mixed_views_device" in rs
    assert "pub struct Lc3GpuInspector" in rs
    # the extents travel with the arrays, in the header's order
    assert re.search(r"lc3gpu_inspector_create\(lc3gpu_inspector \*\*out, int n_streams, const lc3gpu_stream_desc \*descs, int max_views\)", text)
    assert re.search(r"lc3gpu_inspect_mixed_views\(lc3gpu_inspector \*insp, const lc3gpu_view \*views, int n_views, const uint8_t \*d_in, "
                     r"size_t in_bytes,\s*const uint8_t \*d_bad_frame, size_t n_flags, uint8_t \*d_status, size_t n_status, "
                     r"lc3gpu_frame_info \*d_info,\s*size_t n_info, void \*hip_stream\)", text)


def test_the_companion_library_is_built_and_the_main_library_links_it():
    main = pkg.build_native()
    comp = api.inspector_library_path()
    assert os.path.basename(comp) == "liblc3gpu_inspector.so" and os.path.dirname(comp) == os.path.dirname(main)
    assert os.path.exists(comp) and os.path.exists(comp + ".stamp")
    out = subprocess.check_output(["ldd", main], text=True)
    line = [ln for ln in out.splitlines() if "liblc3gpu_inspector.so" in ln]
    assert len(line) == 1 and "not found" not in line[0], out
    assert os.path.realpath(line[0].split("=>")[1].split("(")[0].strip()) == os.path.realpath(comp)  # (found through $ORIGIN: beside the main library)
    dyn = subprocess.check_output(["readelf", "-d", main], text=True)
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn), dyn
    # the companion needs nothing of the main library, and holds the host side under names of its own
    assert "liblc3gpu.so" not in subprocess.check_output(["ldd", comp], text=True)
    C = ctypes.CDLL(comp)
    for name in ("lc3insp_create", "lc3insp_destroy", "lc3insp_mixed_views", "lc3insp_plan_info"):
        assert hasattr(C, name), name
    for name in SYMBOLS:
        assert not hasattr(C, name), name
    # the sources: a host-only unit in the main library, the device code in a unit of its own, the check and plan in a shared header
    assert any(p.endswith("lc3gpu_inspector_api.cpp") for p in api._HOST_SRCS)
    assert "__global__" not in _read("lc3-codec_amd", "csrc", "lc3gpu_inspector_api.cpp")
    assert "inspect_mixed_views" not in _read("lc3-codec_amd", "csrc", "lc3gpu.hip") and "inspector" not in _read("lc3-codec_amd", "csrc", "lc3gpu.hip")
    hip = _read("lc3-codec_amd", "csrc", "lc3gpu_inspector.hip")
    assert '#include "lc3_dev_dec_inspect.h"' in hip and '#include "lc3_host_inspect_views.h"' in hip and "lc3_inspect_record(" in hip
    assert '#include "../../lc3-codec_amd/csrc/lc3_host_inspect_views.h"' in _read("tests", "emu", "lc3_emu_inspect_views.cpp")
    # the inspector's own unit is no part of what the other units are stamped with; the check and plan, and the upload ring, are shared by
    # the companions and hidden from the main units
    own = set(api.companion_own("inspector"))
    assert own == {"lc3gpu_inspector.hip"} and set(api._COMPANION_SHARED) == {"lc3_host_inspect_views.h", "lc3_host_ring.h"}
    names = lambda paths: {os.path.basename(p) for p in paths}
    assert own <= names(api.companion_sources("inspector"))
    for other in api._COMPANIONS:
        assert other == "inspector" or not own & names(api.companion_sources(other)), other
        assert set(api._COMPANION_SHARED) <= names(api.companion_sources(other)), other
    assert not (own | set(api._COMPANION_SHARED)) & names(api.main_sources())
    assert {"lc3gpu.hip", "lc3_dev_common.h", "lc3gpu.h", "lc3_tables.h"} <= names(api.main_sources())


def test_the_header_states_the_refusal_table_and_the_two_equivalences():
    text = " ".join(re.sub(r"\n \*(?= )", " ", _header()).split())  # (a comment's lines joined: no " * " inside a sentence)
    m = re.search(r"Frame inspection over a list of VIEWS(.*?)typedef struct lc3gpu_inspector", text)
    assert m, "the contract of the inspector"
    c = m.group(1)
    for what in ("lc3gpu_decode_mixed_views", "needs no codec handle", "INSPECTOR", "lc3gpu_decoder_create_mixed", "8 kHz included", "7500 or 10000",
                 "1..400", "max_views >= 1", "bound to the device that is current at creation", "not thread-safe", "independent of every codec handle",
                 "LC3GPU_ENODEVICE", "HOST lc3gpu_view[n_views]", "NOT read: pcm_stride, pcm_off, pcm_pitch", "is not refused here",
                 "d_in[byte_off + t * byte_pitch", "d_bad_frame[flag_off + t * flag_pitch]", "d_status[flag_off + t * flag_pitch]",
                 "d_info[flag_off + t * flag_pitch]", "a pitch of 0 stands for the compact one", "At least one of d_status and d_info",
                 "left as it was", "MAY be named by several views", "a ring that wraps", "unspecified", "inside the checked extents",
                 # the two equivalences
                 "byte for byte, the record lc3gpu_inspect writes", "slot_bytes = nb, d_nbytes = NULL", "LC3GPU_FRAME_EMPTY therefore cannot occur",
                 "the status byte is that record's `status`", "status != 0 exactly for the frames lc3gpu_decode_mixed_views conceals",
                 "pair-give-up exception",
                 # the refusal table
                 "launched nothing and written nothing", "channel outside [0, n_streams) LC3GPU_ECHANNEL", "n_frames < 1 LC3GPU_ELENGTH",
                 "nbytes not 0 and outside 1..400 LC3GPU_ELENGTH", "more than 2^31 - 1 frames in one call LC3GPU_ELENGTH",
                 "n_views > max_views LC3GPU_ELENGTH", "[0, in_bytes), [0, n_flags), [0, n_status), [0, n_info) LC3GPU_ELENGTH",
                 "a negative byte_off or flag_off LC3GPU_EINVAL", "a non-zero pitch below its minimum (nb, 1) LC3GPU_EINVAL",
                 "reserved != 0 LC3GPU_EINVAL", "both outputs NULL LC3GPU_EINVAL", "null insp, views or d_in LC3GPU_EINVAL", "n_views < 0 LC3GPU_EINVAL",
                 "d_info not 4-byte aligned LC3GPU_EINVAL", "overlapping d_in's, d_bad_frame's or the other output's LC3GPU_EINVAL",
                 "n_views == 0 LC3GPU_OK (nothing launched)", "unsigned 64-bit arithmetic that cannot wrap", "only against the arrays that are given",
                 "LC3GPU_EHIP", "asynchronous on hip_stream", "does not synchronise the host", "more calls are in flight than the ring has slots",
                 "ONE launch and ONE upload",
                 # out of scope
                 "NOT provided", "a size per frame within a view", "uniform handles and flat batches (lc3gpu_inspect is theirs)", "pipeline object",
                 "host-resident buffers"):
        assert what in c, what
    design = " ".join(_read("DESIGN.md").split())
    for what in ("lc3gpu_inspect_mixed_views", "liblc3gpu_inspector.so", "lc3_iviews_check", "lc3_iviews_build", "lc3_inspect_views_kernel"):
        assert what in design, what
    assert "lc3gpu_inspect_mixed_views" in " ".join(_read("INTEGRATION.md").split()) and "inspect_mixed_views" in _read("README.md")


def test_the_argument_errors_that_need_no_device():
    pkg.build_native()
    L = pkg.load_library()
    h = ctypes.c_void_p()
    descs = api._desc_array([(48000, 10000, 40), (8000, 7500, 20)])
    create = lambda d, n, mv, out=h: L.lc3gpu_inspector_create(ctypes.byref(out) if out is not None else None, n, d, mv)
    assert create(descs, 2, 0) == EINVAL and create(descs, 0, 8) == EINVAL and create(None, 2, 8) == EINVAL
    assert L.lc3gpu_inspector_create(None, 2, descs, 8) == EINVAL
    assert create(api._desc_array([(48000, 5000, 40)]), 1, 8) == EINVAL and create(api._desc_array([(22050, 10000, 40)]), 1, 8) == EINVAL
    assert create(api._desc_array([(48000, 10000, 0)]), 1, 8) == ELENGTH and create(api._desc_array([(48000, 10000, 401)]), 1, 8) == ELENGTH
    assert h.value is None
    views = api._view_list([(0, 2, 0, 1, 0, 0, 0)])
    dev = ctypes.c_void_p(256)  # never dereferenced: the inspector is checked first
    assert L.lc3gpu_inspect_mixed_views(None, views.ctypes.data_as(ctypes.c_void_p), 1, dev, 4096, None, 0, dev, 4096, None, 0, None) == EINVAL
    assert L.lc3gpu_inspector_destroy(None) == EINVAL
    if pkg.device_count() == 0:  # no GPU here: creating an inspector fails loudly
        assert create(descs, 2, 8) == ENODEVICE and h.value is None
        try:
            api.Lc3Inspector([(48000, 10000, 40)], 4)
            assert False, "an inspector without a device"
        except pkg.Lc3GpuError as e:
            assert e.code == ENODEVICE


def test_the_python_layer_sizes_the_record_array_in_records():
    """n_info is in records, not elements: a uint8 buffer of 128 * n bytes is n records"""
    src = _read("lc3-codec_amd", "api.py")
    assert "FRAME_INFO_DTYPE.itemsize" in src[src.index("class Lc3Inspector"):src.index("class PinnedBuffer")]
    assert np.dtype(api.FRAME_INFO_DTYPE).itemsize == 128
