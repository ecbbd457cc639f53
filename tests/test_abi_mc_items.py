"""The C ABI of the multi-channel items calls on mixed-configuration handles (lc3gpu_encode_mixed_mc_items / lc3gpu_decode_mixed_mc_items:
WAV sample order in, frame order out): declared in include/lc3gpu.h with the 16-byte lc3gpu_mc_item, exported by the built library, bound
by the Python layer, the C++ facade and the Rust binding, stated in the header with the contract's differences from the items calls, and
refusing on the host what needs no device.  No GPU needed."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")

SYMBOLS = ["lc3gpu_encode_mixed_mc_items", "lc3gpu_decode_mixed_mc_items"]
EINVAL = -1


def _header():
    with open(os.path.join(ROOT, "include", "lc3gpu.h")) as f:
        return f.read()


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_two_symbols_are_declared_exported_and_bound_in_all_four_bindings():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = pkg.load_library()
    hpp, rs = _read("include", "lc3gpu.hpp"), _read("bindings", "lc3gpu.rs")
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/lc3gpu.h"
        assert hasattr(L, name), name + " is not exported by the built library"
        assert name in api.ABI_SYMBOLS, name
        assert name in hpp, name + " has no facade method in include/lc3gpu.hpp"
        assert re.search(r"pub fn %s\(" % name, rs), name + " is not declared in bindings/lc3gpu.rs"
    assert hasattr(api.Lc3Encoder, "encode_mixed_mc_items") and hasattr(api.Lc3Decoder, "decode_mixed_mc_items")
    assert "encode_mixed_mc_items_device" in rs and "decode_mixed_mc_items_device" in rs
    assert "std::vector<lc3gpu_mc_item>" in hpp


def test_the_item_is_sixteen_bytes_with_the_four_fields_in_order():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"typedef struct lc3gpu_mc_item \{(.*?)\} lc3gpu_mc_item;", text, flags=re.S)
    assert m, "lc3gpu_mc_item is not declared in include/lc3gpu.h"
    fields = re.findall(r"int32_t\s+(\w+)\s*;", m.group(1))
    assert fields == ["first_channel", "n_channels", "n_frames", "nbytes"], fields
    assert "sizeof(lc3gpu_mc_item) == 16" in text
    it = api._mc_item_list([(3, 2, 4), (0, 1, 3, 60), np.array([5, 3, 1, 0])])
    assert it.dtype == np.int32 and it.shape == (3, 4) and it.flags["C_CONTIGUOUS"] and it.strides == (16, 4)
    assert it.tolist() == [[3, 2, 4, 0], [0, 1, 3, 60], [5, 3, 1, 0]]
    assert api._mc_item_list([]).shape == (0, 4)
    with pytest.raises(TypeError):
        api._mc_item_list([(1, 2)])
    with pytest.raises(TypeError):
        api._mc_item_list([(1, 2, 2.5)])
    rs = _read("bindings", "lc3gpu.rs")
    m = re.search(r"pub struct Lc3GpuMcItem \{(.*?)\}", rs, flags=re.S)
    assert m and re.findall(r"pub (\w+): i32", m.group(1)) == fields
    assert "size_of::<Lc3GpuMcItem>() == 16" in rs


def test_the_header_states_the_contract():
    text = " ".join(_header().split())
    m = re.search(r"Batch over a list of MULTI-CHANNEL items of a mixed handle(.*?)typedef struct lc3gpu_mc_item", text)
    assert m, "the contract of the mc-items calls"
    c = m.group(1)
    for what in ("WAV sample order", "HOST lc3gpu_mc_item[n_items]", "no channel in two items", "1..8", "LC3GPU_LAYOUT_INTERLEAVED",
                 "sum_{j<i} T_j * nf_j * C_j", "int16[T_i][nf_i][C_i]", "sum_{j<i} T_j * C_j * nb_j", "uint8[T_i][C_i][nb_i]", "sum_{j<i} T_j * C_j,",
                 "uint8[T_i][C_i]", "nf is even", "2-byte aligned", "16-bit accesses", "LC3GPU_ECHANNEL", "LC3GPU_EINVAL", "LC3GPU_ELENGTH",
                 "LC3GPU_EPAIR", "LC3GPU_EUNSUPPORTED", "differ in fs_hz", "frame_us (lc3_encoder.rs:117-124", "20..400", "1..400", "2^31 - 1 channel-frames",
                 "consumed no pending reset", "lists it alone", "de-interleaved buffers", "every n_channels is 1", "byte for byte", "may alternate",
                 "per 24 buckets", "channel count is not part of the key", "a size per frame", "host-resident", "pipeline object", "uniform handles"):
        assert what in c, what
    # the existing NOT-provided lists point at the new calls
    l = re.search(r"NOT provided by the mixed-list calls \(out of scope\):(.*?)\*/", text).group(1)
    assert "lc3gpu_encode_mixed_mc_items" in l
    l = re.search(r"NOT provided \(out of scope\): a size per FRAME within an item(.*?)\*/", text).group(1)
    assert "lc3gpu_encode_mixed_mc_items" in l
    design = " ".join(_read("DESIGN.md").split())
    assert "lc3gpu_encode_mixed_mc_items" in design and "lc3_mcitems_build" in design


def test_the_version_and_the_argument_errors_that_need_no_device():
    L = pkg.load_library()
    assert L.lc3gpu_version() >= 330
    items = np.array([(0, 2, 1, 0), (2, 1, 2, 40)], np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    dev = ctypes.c_void_p(256)  # never dereferenced: the handle is checked first
    assert L.lc3gpu_encode_mixed_mc_items(None, p(items), 2, dev, dev, None) == EINVAL
    assert L.lc3gpu_decode_mixed_mc_items(None, p(items), 2, dev, None, dev, None) == EINVAL
    assert L.lc3gpu_encode_mixed_mc_items(None, p(items), 0, dev, dev, None) == EINVAL  # (a null handle even with no items)
    assert L.lc3gpu_decode_mixed_mc_items(None, None, -1, dev, None, dev, None) == EINVAL
