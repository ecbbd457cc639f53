"""The C ABI of the items calls on mixed-configuration handles (lc3gpu_encode_mixed_items / lc3gpu_decode_mixed_items: a frame count and a
frame size per listed stream): declared in include/lc3gpu.h with the 16-byte lc3gpu_item, exported by the built library, bound by the
Python layer, the C++ facade and the Rust binding, stated in the header with the contract's differences from the mixed-list calls, and
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

SYMBOLS = ["lc3gpu_encode_mixed_items", "lc3gpu_decode_mixed_items"]
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
    assert hasattr(api.Lc3Encoder, "encode_mixed_items") and hasattr(api.Lc3Decoder, "decode_mixed_items")


def test_the_item_is_sixteen_bytes_in_every_binding():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"typedef struct lc3gpu_item \{(.*?)\} lc3gpu_item;", text, flags=re.S)
    assert m, "lc3gpu_item is not declared in include/lc3gpu.h"
    fields = re.findall(r"int32_t\s+(\w+)\s*;", m.group(1))
    assert fields == ["channel", "n_frames", "nbytes", "reserved"], fields
    assert "sizeof(lc3gpu_item) == 16" in text
    # the Python layer hands the library rows of four int32
    it = api._item_list([(3, 2), (1, 4, 60), np.array([7, 1, 0, 0])])
    assert it.dtype == np.int32 and it.shape == (3, 4) and it.flags["C_CONTIGUOUS"] and it.strides == (16, 4)
    assert it.tolist() == [[3, 2, 0, 0], [1, 4, 60, 0], [7, 1, 0, 0]]
    assert api._item_list([]).shape == (0, 4)
    with pytest.raises(TypeError):
        api._item_list([(1,)])
    with pytest.raises(TypeError):
        api._item_list([(1, 2.5)])
    with open(os.path.join(ROOT, "bindings", "lc3gpu.rs")) as f:
        rs = f.read()
    m = re.search(r"pub struct Lc3GpuItem \{(.*?)\}", rs, flags=re.S)
    assert m and re.findall(r"pub (\w+): i32", m.group(1)) == fields
    assert "size_of::<Lc3GpuItem>() == 16" in rs


def test_the_other_bindings_carry_the_calls():
    with open(os.path.join(ROOT, "include", "lc3gpu.hpp")) as f:
        hpp = f.read()
    with open(os.path.join(ROOT, "bindings", "lc3gpu.rs")) as f:
        rs = f.read()
    for name in SYMBOLS:
        assert name in hpp, name + " has no facade method in include/lc3gpu.hpp"
        assert re.search(r"pub fn %s\(" % name, rs), name + " is not declared in bindings/lc3gpu.rs"
    assert "encode_mixed_items_device" in rs and "decode_mixed_items_device" in rs


def test_the_header_states_the_contract():
    text = " ".join(_header().split())
    m = re.search(r"Batch over a list of ITEMS of a mixed handle(.*?)typedef struct lc3gpu_item", text)
    assert m, "the contract of the items calls"
    c = m.group(1)
    for what in ("HOST lc3gpu_item[n_items]", "no channel twice", "sum_{j<i} n_frames_j * nf_j", "sum_{j<i} n_frames_j * nbytes_j", "one per frame",
                 "nf is even", "LC3GPU_ECHANNEL", "LC3GPU_ELENGTH", "LC3GPU_EINVAL", "LC3GPU_EPAIR", "LC3GPU_EUNSUPPORTED", "20..400", "1..400",
                 "consumed no pending reset", "byte for byte", "may alternate", "per 24 buckets", "a size per FRAME within an item",
                 "interleaved layout", "host-resident", "pipeline object", "uniform handles"):
        assert what in c, what
    # the mixed-list calls no longer list a frame count per listed channel as not provided: they point at the items calls
    l = re.search(r"NOT provided by the mixed-list calls \(out of scope\):(.*?)\*/", text).group(1)
    assert "lc3gpu_encode_mixed_items" in l
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = " ".join(f.read().split())
    assert "lc3gpu_encode_mixed_items" in design and "one launch per kernel per 24 buckets" in design


def test_argument_errors_that_need_no_device():
    L = pkg.load_library()
    items = np.array([(0, 1, 0, 0), (1, 2, 40, 0)], np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    dev = ctypes.c_void_p(256)  # never dereferenced: the handle is checked first
    assert L.lc3gpu_encode_mixed_items(None, p(items), 2, dev, dev, None) == EINVAL
    assert L.lc3gpu_decode_mixed_items(None, p(items), 2, dev, None, dev, None) == EINVAL
    assert L.lc3gpu_encode_mixed_items(None, p(items), 0, dev, dev, None) == EINVAL  # (a null handle even with no items)
    assert L.lc3gpu_decode_mixed_items(None, None, -1, dev, None, dev, None) == EINVAL
