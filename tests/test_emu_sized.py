"""A frame size per frame (lc3gpu_encode_vbr) through the device headers under the CPU wave emulator: the sized front half, back half and
packer (tests/emu/lc3_emu_sized.cpp: the bodies of the sized front and back kernels, the packer frame by frame) against the oracle fed frame by frame with
Encoder.encode_frame(pcm, nbytes) -- the reference's per-call contract.  Four streams per emulated workgroup with different sizes in the
same frame: a size-dependent branch around a workgroup barrier deadlocks the emulator, so every run goes in a subprocess with a time limit."""
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "liblc3emu_sized.so")
synth = importlib.import_module("lc3-codec_amd.synth")
TIME_LIMIT = 900


def _build():
    srcs = [os.path.join(EMU_DIR, "lc3_emu_sized.cpp"), os.path.join(EMU_DIR, "lc3_emu.cpp"), os.path.join(ROOT, "tables", "lc3_tables.h")]
    csrc = os.path.join(ROOT, "lc3-codec_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in srcs):
        return LIB
    tmp = LIB + ".tmp%d" % os.getpid()
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-strict-aliasing",
                           "-Wno-unknown-pragmas", "-Wno-attributes", "-o", tmp, srcs[0], "-lpthread"])
    os.replace(tmp, LIB)
    return LIB


_CHILD = r"""
import ctypes, sys
import numpy as np
lib, fs, us, slot, path = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
z = np.load(path)
pcm, nb = np.ascontiguousarray(z["pcm"]), np.ascontiguousarray(z["nb"])
S, T = nb.shape
out = np.full((S, T, slot), 0xA5, np.uint8)
clamps = ctypes.c_ulonglong(0)
L = ctypes.CDLL(lib)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
rc = L.lc3emu_encode_sized(fs, us, slot, S, T, p(pcm), p(nb), p(out), ctypes.byref(clamps))
np.savez(path, out=out, clamps=np.array([clamps.value, rc], np.int64))
"""


def emu_encode_sized(pcm, nb, slot, fs_hz=48000, frame_us=10000):
    """bytes uint8[S][T][slot] (0xA5 beyond every frame's size), clamp count -- in a child process with a time limit"""
    lib = _build()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "io.npz")
        np.savez(path, pcm=np.ascontiguousarray(pcm, np.int16), nb=np.ascontiguousarray(nb, np.uint16))
        try:
            r = subprocess.run([sys.executable, "-c", _CHILD, lib, str(fs_hz), str(frame_us), str(slot), path], timeout=TIME_LIMIT,
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.fail("sized emulator run did not finish in %d s: a frame-size-dependent branch around a workgroup barrier?" % TIME_LIMIT)
        assert r.returncode == 0, r.stderr[-2000:]
        z = np.load(path)
        assert int(z["clamps"][1]) == 0
        return z["out"], int(z["clamps"][0])


def oracle_sized(pcm, nb, slot, fs_hz=48000, frame_us=10000):
    S, T, _ = pcm.shape
    out = np.full((S, T, slot), 0xA5, np.uint8)
    for s in range(S):
        enc = O.Encoder(fs_hz, frame_us)
        for t in range(T):
            n = int(min(max(int(nb[s, t]), 20), slot))
            out[s, t, :n] = enc.encode_frame(pcm[s, t], n)
    return out


def _material(fs_hz, nf, S, T):
    """the LTPF material's three streams (make_ltpf_pcm) first, then synthetic streams"""
    lt = synth.make_ltpf_pcm(nf, fs_hz, n_frames=T)
    x = synth.make_pcm(S, T, nf, fs_hz)
    x[: min(3, S)] = lt[: min(3, S)]
    return x


def _check(pcm, nb, slot, fs_hz=48000, frame_us=10000):
    got, clamps = emu_encode_sized(pcm, nb, slot, fs_hz, frame_us)
    ref = oracle_sized(pcm, nb, slot, fs_hz, frame_us)
    bad = np.argwhere((got != ref).any(axis=2))
    assert bad.size == 0, "frames (stream, frame) differing from the oracle: %s" % bad[:10].tolist()
    return clamps


# sizes across every border the size enters: lpc_weighting (60 bytes at 10 ms), the attack detector (75 / 100 / 150), gain_ltpf_on (110)
BORDERS_10 = [20, 40, 59, 60, 61, 74, 75, 99, 100, 109, 110, 111, 149, 150, 151, 200, 400]
# 7.5 ms: lpc_weighting 45 bytes, attack detector 75 / 150, gain_ltpf_on 83 bytes (880 bits at 10 ms)
BORDERS_75 = [20, 44, 45, 46, 74, 75, 82, 83, 84, 100, 149, 150, 151, 300]


@pytest.mark.parametrize("T", [3, 4, 5, 9])
def test_sized_encode_48k_10ms_four_sizes_per_frame(T):
    nf, slot = 480, 400
    rng = np.random.default_rng([7, T])
    S = 5  # a full workgroup and a partial one
    pcm = _material(48000, nf, S, T)
    nb = rng.choice(BORDERS_10, size=(S, T)).astype(np.uint16)
    nb[:4, 0] = [60, 110, 150, 75]  # four sizes in one frame of one workgroup
    assert _check(pcm, nb, slot) == 0


def test_sized_encode_48k_7_5ms():
    nf, slot, S, T = 360, 300, 4, 7
    rng = np.random.default_rng(11)
    pcm = _material(48000, nf, S, T)
    nb = rng.choice(BORDERS_75, size=(S, T)).astype(np.uint16)
    assert _check(pcm, nb, slot, 48000, 7500) == 0


def test_sized_encode_ltpf_skip_rule_across_110_bytes():
    # the streams of one workgroup switch between "filter off" (>= 110 bytes) and "filter on" at different frames: frame t's normalised
    # correlation may be skipped only where every stream keeps the filter off at t, t + 1 and t + 2
    nf, slot, T = 480, 200, 12
    pcm = _material(48000, nf, 4, T)
    hi, lo = 150, 100
    nb = np.full((4, T), hi, np.uint16)
    nb[0, 5:7] = lo
    nb[1, 2] = lo
    nb[1, 9:] = lo
    nb[2, ::3] = lo
    nb[3, 7] = 109
    nb[3, 8] = 110
    assert _check(pcm, nb, slot) == 0


def test_sized_encode_clamps_out_of_range_sizes():
    nf, slot, S, T = 480, 120, 4, 3
    pcm = _material(48000, nf, S, T)
    nb = np.array([[0, 7, 19], [121, 60, 120], [20, 500, 110], [65535, 100, 1]], np.uint16)
    assert _check(pcm, nb, slot) == 7  # 0, 7, 19, 121, 500, 65535, 1
