"""Batch calls over VIEWS of a mixed handle (lc3gpu_encode_mixed_views / lc3gpu_decode_mixed_views: every item with the placement of its
PCM, its frames and its flags) through the device headers under the CPU wave emulator.  tests/emu/lc3_emu_views.cpp builds every plan
with lc3_mviews_build and checks every call with lc3_mviews_check of lc3_host_mixed_list.h -- the header the library's host side uses --
and runs the two stream bodies with a stride and a frame pitch, lc3_list_front_stream_view and lc3_list_synth_stream_view of
lc3_dev_list.h, as the view kernels call them.

Host only: the plan for compact placements against lc3_mitems_build (buckets, launch positions, offsets); the plan for placements that
spell out an mc layout against lc3_mcitems_build, by the SETS of addresses the rows reach for every (t, n); every refusal of the
contract's table with its code, the overflow cases among them.

Bodies: one 48 kHz / 10 ms and one 24 kHz / 7.5 ms stream, two ticks of 3 frames, placed with pcm_pitch = nf + 34 at stride 1 and with
pcm_pitch = 2 * nf + 6 at stride 2, frames behind a header at byte_pitch = nbytes + 5, flags 3 apart.  The yardstick is one oracle
encoder / decoder per stream, frame by frame: exact bytes, exact PCM, and every element of the buffers outside the frames' own bytes and
samples still holding its sentinel.  Frames of a view are not contiguous, so a body that takes the MDCT history from frame - (nf - z)
reads the gap's sentinels and misses the oracle's bytes from frame 1 on."""
import ctypes
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
LIB = os.path.join(EMU_DIR, "liblc3emu_views.so")
api = importlib.import_module("lc3-codec_amd.api")
synth = importlib.import_module("lc3-codec_amd.synth")
TIME_LIMIT = 900
OK, EINVAL, ECHANNEL, ELENGTH = 0, -1, -2, -3
FS_ORDER = [8000, 16000, 24000, 32000, 44100, 48000]
A, B, C = (48000, 10000, 100), (48000, 7500, 80), (16000, 10000, 40)
vp, i32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64


def _build():
    srcs = [os.path.join(EMU_DIR, f) for f in ("lc3_emu_views.cpp", "lc3_emu_mc_items.cpp", "lc3_emu_items.cpp", "lc3_emu_mixed_list.cpp", "lc3_emu.cpp")]
    srcs.append(os.path.join(ROOT, "tables", "lc3_tables.h"))
    csrc = os.path.join(ROOT, "lc3-codec_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in srcs):
        return LIB
    tmp = LIB + ".tmp%d" % os.getpid()
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-strict-aliasing",
                           "-Wno-unknown-pragmas", "-Wno-attributes", "-o", tmp, srcs[0], "-lpthread"])
    os.replace(tmp, LIB)
    return LIB


def _lib():
    L = ctypes.CDLL(_build())
    L.lc3emu_ml_new.restype = vp
    L.lc3emu_ml_new.argtypes = [i32, vp]
    L.lc3emu_ml_free.argtypes = [vp]
    L.lc3emu_it_plan.argtypes = [vp, vp, i32, vp, i32, vp, vp]
    L.lc3emu_mc_plan.argtypes = [vp, vp, i32, vp, i32, vp]
    L.lc3emu_vw_plan.argtypes = [vp, vp, i32, i32, vp, i32, vp]
    L.lc3emu_vw_check.argtypes = [vp, vp, i32, u64, u64, u64, u64, i32, i32]
    return L


p = lambda a: a.ctypes.data_as(vp)


def _nf(d):
    return O.Encoder(d[0], d[1]).nf


def test_the_view_and_the_row_sizes():
    L = _lib()
    assert L.lc3emu_vw_view_size() == 64 == api.VIEW_DTYPE.itemsize
    assert L.lc3emu_vw_row_size() == 40, "three 64-bit offsets, the stride and three pitches"


def test_compact_placements_give_the_items_plan():
    """launch positions, buckets and offsets of lc3_mitems_build"""
    L = _lib()
    descs = [A, A, B, C, A, B, C, C, A]
    h = L.lc3emu_ml_new(len(descs), p(np.array(descs, np.int32)))
    try:
        items = [(2, 4, 0), (0, 3, 0), (7, 3, 0), (4, 3, 60), (5, 4, 0), (8, 2, 0), (3, 3, 0), (1, 3, 0), (6, 1, 33)]
        n = len(items)
        it = np.array([r + (0,) for r in items], np.int32)
        rows_it, pos_it, tab_it = np.zeros((16, 8), np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.int64)
        nb = L.lc3emu_it_plan(h, p(it), n, p(rows_it), 16, p(pos_it), p(tab_it))
        assert nb >= 5
        po = bo = fo = 0
        views = []
        for c, T, nbytes in items:  # the items call's prefix sums, stride 1, all pitches 0
            views.append((c, T, nbytes, 1, po, bo, fo))
            po, bo, fo = po + T * _nf(descs[c]), bo + T * (nbytes or descs[c][2]), fo + T
        v = api._view_list(views)
        rows_vw, tab_vw = np.zeros((16, 8), np.int32), np.zeros((n, 8), np.int64)
        assert L.lc3emu_vw_plan(h, p(v), n, 1, p(rows_vw), 16, p(tab_vw)) == nb
        assert np.array_equal(rows_vw[:nb], rows_it[:nb]), "buckets and rows"
        assert tab_vw[:, 0].tolist() == pos_it.tolist(), "launch positions"
        assert np.array_equal(tab_vw[:, 1:4], tab_it), "offsets"
        for k, (c, T, nbytes) in enumerate(items):  # the resolved pitches are the compact ones
            assert tab_vw[k, 4:].tolist() == [1, _nf(descs[c]), nbytes or descs[c][2], 1]
        # without flags the rows' flag fields are 0 / 1 whatever the views hold
        assert L.lc3emu_vw_plan(h, p(v), n, 0, p(rows_vw), 16, p(tab_vw)) == nb
        assert not tab_vw[:, 3].any() and (tab_vw[:, 7] == 1).all()
    finally:
        L.lc3emu_ml_free(h)


def test_views_spelling_out_an_mc_layout_address_what_the_mc_rows_address():
    L = _lib()
    descs = [A, A, A, B, B, C, A]
    h = L.lc3emu_ml_new(len(descs), p(np.array(descs, np.int32)))
    try:
        mc = [(3, 2, 4, 0), (0, 3, 3, 70), (5, 1, 2, 0), (6, 1, 3, 0)]
        n_ch = sum(C_ for _, C_, _, _ in mc)
        rows_mc, tab_mc = np.zeros((16, 8), np.int32), np.zeros((n_ch, 5), np.int64)
        nb = L.lc3emu_mc_plan(h, p(np.array(mc, np.int32)), len(mc), p(rows_mc), 16, p(tab_mc))
        views, P = [], [0, 0, 0]
        for first, C_, T, nbytes in mc:
            nf, size = _nf(descs[first]), nbytes or descs[first][2]
            for c in range(C_):
                views.append((first + c, T, nbytes, C_, P[0] + c, P[1] + c * size, P[2] + c, nf * C_, C_ * size, C_))
            P = [P[0] + T * nf * C_, P[1] + T * C_ * size, P[2] + T * C_]
        v = api._view_list(views)
        rows_vw, tab_vw = np.zeros((16, 8), np.int32), np.zeros((n_ch, 8), np.int64)
        assert L.lc3emu_vw_plan(h, p(v), n_ch, 1, p(rows_vw), 16, p(tab_vw)) == nb
        assert np.array_equal(rows_vw[:nb], rows_mc[:nb]) and tab_vw[:, 0].tolist() == tab_mc[:, 0].tolist()
        for k, view in enumerate(views):
            ch, T = view[0], view[1]
            nf, size = _nf(descs[ch]), view[2] or descs[ch][2]
            _, m_pcm, m_byte, m_flag, m_C = tab_mc[k].tolist()
            _, pcm_off, byte_off, flag_off, stride, pp, bp, fp = tab_vw[k].tolist()
            t, s = np.arange(T)[:, None], np.arange(nf)[None, :]
            assert np.array_equal(pcm_off + t * pp + s * stride, m_pcm + (t * nf + s) * m_C), "samples of channel %d" % ch
            b = np.arange(size)[None, :]
            assert np.array_equal(byte_off + t * bp + b, m_byte + t * m_C * size + b), "bytes of channel %d" % ch
            assert np.array_equal(flag_off + t[:, 0] * fp, m_flag + t[:, 0] * m_C), "flags of channel %d" % ch
    finally:
        L.lc3emu_ml_free(h)


def test_every_refusal_gives_its_code():
    L = _lib()
    descs = [A, B, C, A]  # nf 480, 360, 160, 480; 100, 80, 40, 100 bytes
    h = L.lc3emu_ml_new(len(descs), p(np.array(descs, np.int32)))
    PCM, IO, FL = 1 << 20, 1 << 16, 64
    base = [dict(channel=0, n_frames=3, pcm_off=0, byte_off=0, flag_off=0),
            dict(channel=1, n_frames=4, pcm_off=4000, byte_off=1000, flag_off=8, pcm_stride=2, byte_pitch=412, flag_pitch=2),
            dict(channel=2, n_frames=1, pcm_off=9000, byte_off=4000, flag_off=20, nbytes=64)]

    def check(views, pcm_base=0x1000, pcm=PCM, io=IO, fl=FL, use=1, mn=20):
        v = api._view_list(views)
        return L.lc3emu_vw_check(h, p(v) if len(v) else None, len(v), pcm_base, pcm, io, fl, use, mn)

    def with_(k, **kw):
        out = [dict(d) for d in base]
        out[k].update(kw)
        return out

    try:
        assert check(base) == OK and check(base, use=0, fl=0) == OK and check([]) == OK
        for bad in (with_(0, channel=-1), with_(0, channel=4), with_(2, channel=1)):
            assert check(bad) == ECHANNEL
        for bad in (with_(0, n_frames=0), with_(1, n_frames=-3), with_(0, nbytes=401), with_(0, nbytes=-1), with_(0, nbytes=19)):
            assert check(bad) == ELENGTH
        assert check(with_(0, nbytes=19), mn=1) == OK and check(with_(0, nbytes=1), mn=1) == OK  # the decoder takes 1..19
        for bad in (with_(0, pcm_stride=0), with_(0, pcm_stride=9), with_(0, pcm_stride=-1)):
            assert check(bad) == EINVAL
        for bad in (with_(0, pcm_off=-2), with_(1, byte_off=-1), with_(2, flag_off=-1)):
            assert check(bad) == EINVAL
        assert check(with_(2, flag_off=-1), use=0) == OK, "flag placement is ignored when no flags are read"
        for bad in (with_(0, pcm_pitch=478), with_(1, pcm_pitch=2 * 360 - 1), with_(0, byte_pitch=99), with_(2, byte_pitch=63), with_(0, flag_pitch=-1),
                    with_(0, pcm_pitch=-480), with_(0, byte_pitch=-100)):
            assert check(bad) == EINVAL
        assert check(with_(0, pcm_pitch=480, byte_pitch=100, flag_pitch=1)) == OK  # the minima themselves
        v = api._view_list(base)
        for k in range(3):
            w = v.copy()
            w["reserved"][1][k] = 1
            assert L.lc3emu_vw_check(h, p(w), 3, 0x1000, PCM, IO, FL, 1, 20) == EINVAL
        # the 32-bit path: even offset, even pitch, a 4-byte aligned base; the 16-bit path: a 2-byte aligned base
        assert check(with_(0, pcm_off=1)) == EINVAL and check(with_(0, pcm_pitch=481)) == EINVAL and check(base[:1], pcm_base=0x1002) == EINVAL
        assert check(with_(1, pcm_off=4001, pcm_pitch=721)) == OK and check(base[1:2], pcm_base=0x1002) == OK
        assert check(base[1:2], pcm_base=0x1001) == EINVAL
        # extents: the last sample / byte / flag exactly at the buffer's end is accepted, one further is refused
        one = lambda **kw: [dict(dict(channel=0, n_frames=3, pcm_off=0, byte_off=0, flag_off=0), **kw)]
        last_pcm = 10 + 2 * 500 + 479
        assert check(one(pcm_off=10, pcm_pitch=500), pcm=last_pcm + 1) == OK and check(one(pcm_off=10, pcm_pitch=500), pcm=last_pcm) == ELENGTH
        last_pcm = 3 + 2 * 3900 + 479 * 8
        assert check(one(pcm_off=3, pcm_stride=8, pcm_pitch=3900), pcm=last_pcm + 1) == OK
        assert check(one(pcm_off=3, pcm_stride=8, pcm_pitch=3900), pcm=last_pcm) == ELENGTH
        last_byte = 12 + 2 * 412 + 99
        assert check(one(byte_off=12, byte_pitch=412), io=last_byte + 1) == OK and check(one(byte_off=12, byte_pitch=412), io=last_byte) == ELENGTH
        assert check(one(byte_off=12, byte_pitch=412, nbytes=400), io=12 + 2 * 412 + 400) == OK
        assert check(one(byte_off=13, byte_pitch=412, nbytes=400), io=12 + 2 * 412 + 400) == ELENGTH
        assert check(one(flag_off=5, flag_pitch=7), fl=20) == OK and check(one(flag_off=5, flag_pitch=7), fl=19) == ELENGTH
        assert check(one(flag_off=5, flag_pitch=7), fl=0, use=0) == OK
        assert check(one(), pcm=0) == ELENGTH and check(one(), io=0) == ELENGTH and check(one(), fl=0) == ELENGTH
        # the overflow cases: offsets near 2^62 and 2^63, a pitch of 2^31 - 1 with many frames
        big = (1 << 62) - 2
        for kw in (dict(pcm_off=big), dict(byte_off=big), dict(flag_off=big), dict(pcm_off=(1 << 63) - 2), dict(byte_off=(1 << 63) - 1)):
            assert check(one(**kw)) == ELENGTH
        assert check(one(pcm_off=big), pcm=big + 2 * 480 + 480) == OK and check(one(pcm_off=big), pcm=big + 2 * 480 + 479) == ELENGTH
        huge, T = (1 << 31) - 1, (1 << 31) - 1
        far = dict(n_frames=T, pcm_pitch=huge - 1, byte_pitch=huge, flag_pitch=huge)
        assert check(one(**far)) == ELENGTH
        need_pcm, need_io, need_fl = (T - 1) * (huge - 1) + 480, (T - 1) * huge + 100, (T - 1) * huge + 1
        assert check(one(**far), pcm=need_pcm, io=need_io, fl=need_fl) == OK
        assert check(one(**far), pcm=need_pcm - 1, io=need_io, fl=need_fl) == ELENGTH
        assert check(one(**far), pcm=need_pcm, io=need_io - 1, fl=need_fl) == ELENGTH
        assert check(one(**far), pcm=need_pcm, io=need_io, fl=need_fl - 1) == ELENGTH
        top = (1 << 63) - 2  # offset plus span passes 2^63: signed 64-bit arithmetic would wrap to a negative "last element"
        assert check(one(**dict(far, pcm_off=top)), pcm=top + need_pcm, io=need_io, fl=need_fl) == OK
        assert check(one(**dict(far, pcm_off=top)), pcm=top + need_pcm - 1, io=need_io, fl=need_fl) == ELENGTH
        assert check(one(**dict(far, byte_off=top + 1)), pcm=need_pcm, io=top + need_io, fl=need_fl) == ELENGTH
        # more than 2^31 - 1 frames in one call
        two = [dict(channel=0, n_frames=T, pcm_off=0, byte_off=0, flag_off=0), dict(channel=1, n_frames=1, pcm_off=0, byte_off=0, flag_off=0)]
        assert check(two, pcm=1 << 50, io=1 << 50, fl=1 << 50) == ELENGTH
        assert check(two[:1], pcm=1 << 50, io=1 << 50, fl=1 << 50) == OK
    finally:
        L.lc3emu_ml_free(h)


_CHILD = r"""
import ctypes, sys
import numpy as np
lib, path = sys.argv[1], sys.argv[2]
z = np.load(path)
descs = np.ascontiguousarray(z["descs"], np.int32)
n_ch = descs.shape[0]
L = ctypes.CDLL(lib)
vp, i = ctypes.c_void_p, ctypes.c_int
L.lc3emu_ml_new.restype = vp
L.lc3emu_ml_new.argtypes = [i, vp]
L.lc3emu_vw_encode.argtypes = [vp, vp, i, vp, vp, vp, vp]
L.lc3emu_vw_decode.argtypes = [vp, vp, i, vp, vp, vp, vp, i, vp]
L.lc3emu_ml_free.argtypes = [vp]
p = lambda a: a.ctypes.data_as(vp)
res = {}
for run in range(int(z["n_runs"])):
    h = L.lc3emu_ml_new(n_ch, p(descs))
    assert h
    for k in range(int(z["n_ticks"])):
        key = "%d_%d" % (run, k)
        views = np.ascontiguousarray(z["views_" + key])
        fresh = np.full(n_ch, int(k == 0), np.uint8)
        info = np.zeros(8, np.int32)
        out = np.ascontiguousarray(z["out_" + key])
        assert L.lc3emu_vw_encode(h, p(views), views.shape[0], p(fresh), p(np.ascontiguousarray(z["pcm_" + key])), p(out), p(info)) == 0
        assert info[0] == 0, "plane columns outside the call's frames were written"
        res["bytes_" + key] = out
        pcm_out = np.ascontiguousarray(z["pcm_out_" + key])
        assert L.lc3emu_vw_decode(h, p(views), views.shape[0], p(fresh), p(np.ascontiguousarray(z["in_" + key])), p(np.ascontiguousarray(z["bad_" + key])),
                                  p(pcm_out), int(z["late_%d" % run]), p(info)) == 0
        assert info[0] == 0
        res["pcm_" + key] = pcm_out
    L.lc3emu_ml_free(h)
np.savez(path, **res)
"""


def test_bodies_with_a_frame_pitch_against_the_oracle():
    descs = [(48000, 10000, 100), (24000, 7500, 60)]
    nf = [_nf(d) for d in descs]
    assert nf == [480, 180]
    T, TICKS = 3, 2
    rng = np.random.default_rng(77)
    material = [synth.make_ltpf_pcm(nf[0], 48000, n_frames=T * TICKS)[0], synth.make_pcm(1, T * TICKS, nf[1], 24000, seed=9)[0]]
    io = {"descs": np.array(descs, np.int32), "n_runs": 2, "n_ticks": TICKS}
    want = {}
    HEADER, BYTE_GAP, FLAG_PITCH = 12, 5, 3
    for run, (stride, late) in enumerate(((1, 0), (2, 1))):
        io["late_%d" % run] = late
        enc_or = [O.Encoder(d[0], d[1]) for d in descs]
        dec_or = [O.Decoder(d[0], d[1]) for d in descs]
        for k in range(TICKS):
            key = "%d_%d" % (run, k)
            pitch = [n + 34 if stride == 1 else 2 * n + 6 for n in nf]
            views, po, bo, fo = [], 6, 0, 1
            for c in (1, 0) if k else (0, 1):  # (list order and launch order differ in one of the ticks)
                views.append(dict(channel=c, n_frames=T, pcm_stride=stride, pcm_off=po + (stride - 1), pcm_pitch=pitch[c], byte_off=bo + HEADER,
                                  byte_pitch=descs[c][2] + BYTE_GAP, flag_off=fo, flag_pitch=FLAG_PITCH))
                po, bo, fo = po + T * pitch[c] + 10, bo + T * (descs[c][2] + BYTE_GAP) + HEADER, fo + T * FLAG_PITCH
            pcm = np.full(po, 12345, np.int16)
            out = np.full(bo, 0xA5, np.uint8)
            flags = np.zeros(fo, np.uint8)
            ref_out, ref_pcm, data = out.copy(), pcm.copy(), out.copy()
            for v in views:
                c = v["channel"]
                for t in range(T):
                    x = material[c][k * T + t]
                    at = v["pcm_off"] + t * v["pcm_pitch"]
                    pcm[at:at + nf[c] * stride:stride] = x
                    fr = enc_or[c].encode_frame(np.ascontiguousarray(x), descs[c][2])
                    b = v["byte_off"] + t * v["byte_pitch"]
                    ref_out[b:b + descs[c][2]] = fr
                    buf = np.array(fr, np.uint8)
                    if rng.random() < 0.25:
                        buf[rng.integers(0, buf.size, 3)] ^= rng.integers(1, 256, 3).astype(np.uint8)
                    data[b:b + descs[c][2]] = buf
                    if rng.random() < 0.2:
                        flags[v["flag_off"] + t * v["flag_pitch"]] = 1
                        buf = buf.copy()
                        buf[-2:] = 0xFF  # (the oracle has no external flag: unparsable side information)
                    _, y = dec_or[c].decode_frame(buf)
                    ref_pcm[at:at + nf[c] * stride:stride] = y
            # flags between the views' own are set: a body that reads flag_off + t instead of + t * flag_pitch conceals the wrong frames
            own = [v["flag_off"] + t * v["flag_pitch"] for v in views for t in range(T)]
            flags[[f for f in range(fo) if f not in own]] = 1
            io["views_" + key] = api._view_list(views)
            io["pcm_" + key], io["out_" + key], io["in_" + key], io["bad_" + key] = pcm, out, data, flags
            io["pcm_out_" + key] = np.full(po, 12345, np.int16)
            want[key] = (ref_out, ref_pcm)
    lib = _build()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "io.npz")
        np.savez(path, **io)
        try:
            r = subprocess.run([sys.executable, "-c", _CHILD, lib, path], timeout=TIME_LIMIT, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.fail("views emulator run did not finish in %d s: a workgroup barrier steered by stride or pitch?" % TIME_LIMIT)
        assert r.returncode == 0, r.stderr[-2000:]
        z = np.load(path)
        for key, (ref_out, ref_pcm) in want.items():
            # the whole buffers: the frames' own bytes / samples are the oracle's, everything else still holds its sentinel
            assert np.array_equal(z["bytes_" + key], ref_out), "run_tick %s: bytes differ from the oracle, or a byte outside the frames was written" % key
            assert np.array_equal(z["pcm_" + key], ref_pcm), "run_tick %s: PCM differs from the oracle, or a sample outside the frames was written" % key
