"""The C ABI of the channel-list calls on mixed-configuration handles (lc3gpu_encode_mixed_list / lc3gpu_decode_mixed_list): declared in
include/lc3gpu.h, exported by the built library, bound by the Python layer, stated in the header with what they leave out, and safe to call
with a null handle (LC3GPU_EINVAL, nothing aborts).  No GPU needed."""
import ctypes
import importlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")

SYMBOLS = ["lc3gpu_encode_mixed_list", "lc3gpu_decode_mixed_list"]
EINVAL = -1


def _header():
    with open(os.path.join(ROOT, "include", "lc3gpu.h")) as f:
        return f.read()


def test_the_two_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = pkg.load_library()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/lc3gpu.h"
        assert hasattr(L, name), name + " is not exported by the built library"
        assert name in api.ABI_SYMBOLS, name
    assert hasattr(api.Lc3Encoder, "encode_mixed_list") and hasattr(api.Lc3Decoder, "decode_mixed_list")


def test_the_other_bindings_carry_the_calls():
    with open(os.path.join(ROOT, "include", "lc3gpu.hpp")) as f:
        hpp = f.read()
    with open(os.path.join(ROOT, "bindings", "lc3gpu.rs")) as f:
        rs = f.read()
    for name in SYMBOLS:
        assert name in hpp, name + " has no facade method in include/lc3gpu.hpp"
        assert re.search(r"pub fn %s\(" % name, rs), name + " is not declared in bindings/lc3gpu.rs"


def test_the_header_states_what_the_mixed_list_calls_leave_out():
    text = " ".join(_header().split())
    m = re.search(r"lc3gpu_encode_mixed_list.*?NOT provided by the mixed-list calls \(out of scope\):(.*?)\*/", text)
    assert m, "the out-of-scope list of the mixed-list calls"
    for what in ("interleaved layout", "frame size per frame", "host-resident", "pipeline", "frame count per listed channel"):
        assert what in m.group(1), what
    # the uniform list calls still refuse mixed handles and say where to go instead
    u = re.search(r"NOT provided \(out of scope\):(.*?)\*/", text)
    assert u and "mixed handles" in u.group(1) and "lc3gpu_encode_mixed_list" in u.group(1)


def test_a_null_handle_is_an_invalid_argument():
    L = pkg.load_library()
    ch = np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    dev = ctypes.c_void_p(256)  # never dereferenced: the handle is checked first
    assert L.lc3gpu_encode_mixed_list(None, p(ch), 4, dev, dev, 1, None) == EINVAL
    assert L.lc3gpu_decode_mixed_list(None, p(ch), 4, dev, None, dev, 1, None) == EINVAL


def test_the_version_went_up_with_the_new_calls():
    assert pkg.load_library().lc3gpu_version() >= 320
