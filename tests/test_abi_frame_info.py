"""The layout of lc3gpu_frame_info (include/lc3gpu.h) is ABI: a C program compiled against the header with gcc reports the size and the
offset of every field, and they must be those of the Python mirror api.FRAME_INFO_DTYPE and of the Rust binding's field list."""
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
api = importlib.import_module("lc3-codec_amd.api")


def _c_layout(tmp_path):
    fields = api.FRAME_INFO_DTYPE.names
    src = tmp_path / "layout.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lc3gpu.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(lc3gpu_frame_info));']
    for f in fields:
        lines.append('    printf("%s %%zu %%zu\\n", offsetof(lc3gpu_frame_info, %s), sizeof(((lc3gpu_frame_info *)0)->%s));' % (f, f, f))
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    size = int(out[0].split()[1])
    layout = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in out[1:] if ln.strip()}
    return size, layout


def test_c_layout_matches_numpy_dtype(tmp_path):
    size, layout = _c_layout(tmp_path)
    dt = api.FRAME_INFO_DTYPE
    assert size == 128 == dt.itemsize
    assert list(layout) == list(dt.names)
    for name in dt.names:
        sub, off = dt.fields[name][:2]
        assert layout[name] == (off, sub.itemsize), name


def test_rust_struct_lists_the_fields_in_order():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rust_binding as G
    finally:
        sys.path.pop(0)
    fields = G.frame_info_fields()
    assert [n for n, _ in fields] == list(api.FRAME_INFO_DTYPE.names)
    width = {"i32": 4, "u32": 4, "u8": 1}
    total = 0
    for _, t in fields:
        if t.startswith("["):
            elem, n = t[1:-1].split(";")
            total += width[elem.strip()] * int(n)
        else:
            total += width[t]
    assert total == 128


@pytest.mark.parametrize("name,value", [("LC3GPU_FRAME_OK", 0), ("LC3GPU_FRAME_FLAGGED", 1), ("LC3GPU_FRAME_EMPTY", 2),
                                        ("LC3GPU_FRAME_SIDE_INFO", 16), ("LC3GPU_FRAME_ARITH", 32)])
def test_status_constants(name, value):
    text = open(os.path.join(ROOT, "include", "lc3gpu.h")).read()
    assert "#define %s %d\n" % (name, value) in text
    assert getattr(api, name[len("LC3GPU_"):]) == value
    assert "pub const %s: i32 = %d;" % (name, value) in open(os.path.join(ROOT, "bindings", "lc3gpu.rs")).read()
