"""lc3gpu_inspect_mixed_views on the CPU (no GPU needed): the check and plan header the companion library runs on the host
(lc3-codec_amd/csrc/lc3_host_inspect_views.h) through tests/emu/lc3_emu_inspect_views.cpp -- every refusal of the header's table with its
code, offsets near 2^62 and 2^63, a pitch of 2^31 - 1 with 2^31 - 1 frames, views ending exactly at each array's end and one element
further, the address-overlap refusals; the plan spelled out lane by lane with the kernel's own look-ups (every (view, frame) in exactly
one lane of exactly one workgroup, every workgroup uniform in configuration and size); and the kernel's lane body driven through the plan
over a tick of all 12 configurations against the oracle's records, whole output arrays compared, sentinels included.  The same extreme
lists go through a stand-alone program built with -fsanitize=address,undefined (tests/emu/lc3_inspect_views_check_main.cpp)."""
import ctypes
import importlib
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import inspect_lib as I
from inspect_views_lib import expected_outputs, tick, view, views_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "liblc3emu_inspect_views.so")
api = importlib.import_module("lc3-codec_amd.api")

OK, EINVAL, ECHANNEL, ELENGTH = 0, -1, -2, -3
DESCS = [(fs, us, 40) for fs, us in I.CONFIGS]
M31 = 2**31 - 1


def _build():
    srcs = [os.path.join(EMU_DIR, "lc3_emu_inspect_views.cpp"), os.path.join(EMU_DIR, "lc3_emu.cpp"), os.path.join(ROOT, "tables", "lc3_tables.h"),
            os.path.join(ROOT, "include", "lc3gpu.h")]
    csrc = os.path.join(ROOT, "lc3-codec_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not (os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in srcs)):
        tmp = LIB + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-strict-aliasing",
                               "-Wno-unknown-pragmas", "-Wno-attributes", "-o", tmp, srcs[0], "-lpthread"])
        os.replace(tmp, LIB)
    L = ctypes.CDLL(LIB)
    L.lc3emu_iv_lds.restype = ctypes.c_longlong
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    L.lc3emu_iv_check.argtypes = [vp, i, i, vp, i, vp, vp]
    L.lc3emu_iv_plan.argtypes = [vp, i, vp, i, i, i, vp, ctypes.c_longlong, vp, i, vp]
    L.lc3emu_iv_run.argtypes = [vp, i, i, vp, i, vp, u64, vp, u64, vp, u64, vp, u64]
    return L


@pytest.fixture(scope="module")
def emu():
    return _build()


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def descs_array(descs):
    return np.ascontiguousarray(np.array(descs, np.int32).reshape(-1, 3))


# in base / bytes, flags base / n, status base / n, info base / n: four arrays far apart
BOUNDS = dict(in_base=0x10000000, in_bytes=1 << 20, flags_base=0x20000000, n_flags=1 << 16, status_base=0x30000000, n_status=1 << 16,
              info_base=0x40000000, n_info=1 << 16)
KEYS = ("in_base", "in_bytes", "flags_base", "n_flags", "status_base", "n_status", "info_base", "n_info")


def bounds(**over):
    b = dict(BOUNDS, **over)
    return np.array([b[k] for k in KEYS], np.uint64)


def cases():
    """(name, views or None, n_views or None (= len), bounds, max_views, want): the header's refusal table and the extremes"""
    C = []

    def add(name, vs, want, n_views=None, max_views=64, **over):
        C.append((name, vs, len(vs) if n_views is None else n_views, bounds(**over), max_views, want))

    one = view(channel=3, n_frames=4, byte_off=12, byte_pitch=412, flag_off=5, flag_pitch=2)
    add("plain", views_of(one), OK)
    add("a view the decode call would refuse for its PCM placement", views_of(view(pcm_stride=99, pcm_off=-7, pcm_pitch=1)), OK)
    add("one channel in two views", views_of(one, view(channel=3, n_frames=2, byte_off=5000, flag_off=100)), OK)
    add("no views", views_of(), OK)
    add("no views, no list", None, EINVAL, n_views=0)
    for ch in (-1, 12, M31):
        add("channel %d" % ch, views_of(view(channel=ch)), ECHANNEL)
    for n in (0, -1, -M31 - 1):
        add("n_frames %d" % n, views_of(view(n_frames=n)), ELENGTH)
    for nb, want in ((-1, ELENGTH), (401, ELENGTH), (M31, ELENGTH), (1, OK), (400, OK)):
        add("nbytes %d" % nb, views_of(view(nbytes=nb)), want)
    add("more views than max_views", views_of(one, one, one), ELENGTH, max_views=2)
    add("as many views as max_views", views_of(one, one), OK, max_views=2)
    add("a negative byte_off", views_of(view(byte_off=-1)), EINVAL)
    add("a negative flag_off", views_of(view(flag_off=-1)), EINVAL)
    add("the most negative offsets", views_of(view(byte_off=-2**63, flag_off=-2**63)), EINVAL)
    add("byte_pitch below the size", views_of(view(n_frames=2, byte_pitch=39)), EINVAL)
    add("byte_pitch below the view's size", views_of(view(n_frames=2, nbytes=100, byte_pitch=99)), EINVAL)
    add("byte_pitch the size", views_of(view(n_frames=2, nbytes=100, byte_pitch=100)), OK)
    add("a negative byte_pitch", views_of(view(n_frames=2, byte_pitch=-412)), EINVAL)
    add("a negative flag_pitch", views_of(view(n_frames=2, flag_pitch=-1)), EINVAL)
    for k in range(3):
        add("reserved[%d]" % k, views_of(view(reserved=tuple(int(j == k) for j in range(3)))), EINVAL)
    add("both outputs NULL", views_of(one), EINVAL, status_base=0, info_base=0)
    add("both outputs NULL, no views", views_of(), EINVAL, status_base=0, info_base=0)
    add("status only", views_of(one), OK, info_base=0, n_info=0)
    add("records only", views_of(one), OK, status_base=0, n_status=0)
    add("no flags", views_of(one), OK, flags_base=0, n_flags=0)
    add("null views", None, EINVAL, n_views=1)
    add("n_views < 0", views_of(one), EINVAL, n_views=-1)
    add("null d_in", views_of(one), EINVAL, in_base=0)
    for mis in (1, 2, 3):
        add("d_info off by %d" % mis, views_of(one), EINVAL, info_base=0x40000000 + mis)
    add("d_info 4-byte aligned", views_of(one), OK, info_base=0x40000004)
    # exactly at each array's end, and one element further
    add("bytes end at the end", views_of(view(n_frames=3, byte_off=12, byte_pitch=412)), OK, in_bytes=12 + 2 * 412 + 40)
    add("bytes end one past", views_of(view(n_frames=3, byte_off=12, byte_pitch=412)), ELENGTH, in_bytes=12 + 2 * 412 + 39)
    add("byte_off at the end", views_of(view(byte_off=1 << 20)), ELENGTH)
    for arr in ("n_flags", "n_status", "n_info"):
        v = views_of(view(n_frames=3, flag_off=7, flag_pitch=5))
        add("%s: the last index is the last element" % arr, v, OK, **{arr: 18})
        add("%s: one further" % arr, v, ELENGTH, **{arr: 17})
        add("%s: flag_off at the end" % arr, views_of(view(flag_off=18)), ELENGTH, **{arr: 18})
    add("flags not given: n_flags is not looked at", views_of(view(n_frames=3, flag_off=7, flag_pitch=5)), OK, flags_base=0, n_flags=1)
    add("status not given: n_status is not looked at", views_of(view(flag_off=7)), OK, status_base=0, n_status=1)
    add("records not given: n_info is not looked at", views_of(view(flag_off=7)), OK, info_base=0, n_info=1)
    add("the second view is the bad one", views_of(one, view(n_frames=3, flag_off=(1 << 16) - 2)), ELENGTH)
    # frame counts
    big = dict(in_base=4096, in_bytes=1 << 40, flags_base=0, n_flags=0, status_base=1 << 62, n_status=1 << 40, info_base=0, n_info=0)
    add("2^31 - 1 frames", views_of(view(n_frames=M31, nbytes=1)), OK, **big)
    add("2^31 frames in two views", views_of(view(n_frames=M31, nbytes=1), view(n_frames=1, nbytes=1)), ELENGTH, **big)
    add("2^32 - 2 frames in two views", views_of(view(n_frames=M31, nbytes=1), view(n_frames=M31, nbytes=1)), ELENGTH, **big)
    # a pitch of 2^31 - 1 with 2^31 - 1 frames: the span is (2^31 - 2) * (2^31 - 1) + the last element
    span = (M31 - 1) * M31
    far = dict(in_base=4096, flags_base=0, n_flags=0, status_base=1 << 63, info_base=0, n_info=0)
    v = views_of(view(n_frames=M31, byte_pitch=M31, flag_pitch=M31))
    add("the longest view fits", v, OK, in_bytes=span + 40, n_status=span + 1, **far)
    add("the longest view: one byte short", v, ELENGTH, in_bytes=span + 39, n_status=span + 1, **far)
    add("the longest view: one status byte short", v, ELENGTH, in_bytes=span + 40, n_status=span, **far)
    add("the longest view from 2^62 on", views_of(view(n_frames=M31, byte_pitch=M31, flag_pitch=M31, byte_off=1 << 62, flag_off=1 << 62)), OK,
        in_bytes=(1 << 62) + span + 40, n_status=(1 << 62) + span + 1, **far)
    # offsets near 2^62 and 2^63
    add("byte_off 2^62 inside", views_of(view(byte_off=1 << 62)), OK, in_bytes=(1 << 62) + 40, **far, n_status=16)
    add("byte_off 2^62: one byte short", views_of(view(byte_off=1 << 62)), ELENGTH, in_bytes=(1 << 62) + 39, **far, n_status=16)
    farther = dict(far, status_base=(1 << 63) + (1 << 62))
    add("byte_off 2^63 - 1 inside", views_of(view(byte_off=2**63 - 1)), OK, in_bytes=2**63 + 39, **farther, n_status=16)
    add("byte_off 2^63 - 1: one byte short", views_of(view(byte_off=2**63 - 1)), ELENGTH, in_bytes=2**63 + 38, **farther, n_status=16)
    add("byte_off 2^63 - 1 with frames beyond 2^63", views_of(view(n_frames=1000, byte_off=2**63 - 1, byte_pitch=M31)), OK,
        in_bytes=2**63 + 999 * M31 + 39, **farther, n_status=1000)
    add("flag_off 2^63 - 1 inside a status array that ends at 2^64", views_of(view(flag_off=2**63 - 1)), OK, n_status=2**63, **far, in_bytes=40)
    add("flag_off 2^63 - 1: one short", views_of(view(flag_off=2**63 - 1)), ELENGTH, n_status=2**63 - 1, **far, in_bytes=40)
    add("flag_off 2^62 in a record array of 2^62 + 1", views_of(view(flag_off=1 << 62)), OK, in_base=4096, in_bytes=40, flags_base=0, n_flags=0,
        status_base=0, n_status=0, info_base=1 << 20, n_info=(1 << 62) + 1)  # (n_info * 128 passes 2^64: the range is taken to the end)
    add("an array that ends at 2^64 - 1", views_of(view(byte_off=2**63 - 1, n_frames=M31, byte_pitch=M31)), OK, in_base=1 << 40,
        in_bytes=2**64 - 1 - (1 << 40), flags_base=0, n_flags=0, status_base=4096, n_status=M31, info_base=0, n_info=0)
    # address overlaps: an output against d_in, d_bad_frame and the other output; touching is no overlap
    S, NS = BOUNDS["status_base"], BOUNDS["n_status"]
    add("status begins inside d_in", views_of(one), EINVAL, in_base=S - 100, in_bytes=101)
    add("status ends where d_in begins", views_of(one), OK, in_base=S + NS, in_bytes=4096)
    add("d_in ends where status begins", views_of(one), OK, in_base=S - 4096, in_bytes=4096)
    add("d_in inside status", views_of(one), EINVAL, in_base=S + 100, in_bytes=1000)
    add("status's last byte is the first flag", views_of(one), EINVAL, flags_base=S + NS - 1)
    add("status is the flag array", views_of(one), EINVAL, flags_base=S, n_flags=NS)
    add("status inside the records", views_of(one), EINVAL, info_base=S - 128)
    add("the records end where status begins", views_of(one), OK, info_base=S - 128 * 64, n_info=64)
    add("the records' last byte is status's first", views_of(one), EINVAL, info_base=S - 128 * 64 + 4, n_info=64)
    add("the records over d_in", views_of(one), EINVAL, info_base=BOUNDS["in_base"] + 4096)
    add("the records over the flags", views_of(one), EINVAL, info_base=BOUNDS["flags_base"] - 128)
    add("the records given, the flags not: no flag range to overlap", views_of(one), OK, info_base=BOUNDS["flags_base"] - 128, flags_base=0)
    add("an output range of no elements overlaps nothing", views_of(), OK, info_base=BOUNDS["in_base"], n_info=0)
    return C


def test_every_refusal_and_every_extreme_has_its_code(emu):
    d = descs_array(DESCS)
    out = np.zeros(2, np.int32)
    seen = set()
    for name, vs, n, b, max_views, want in cases():
        rc = emu.lc3emu_iv_check(P(d), len(DESCS), max_views, P(vs), n, P(b), P(out))
        assert rc == want, (name, rc, want)
        seen.add(want)
        if rc == OK and vs is not None and len(vs):
            assert out[0] == int(vs["n_frames"].astype(np.int64).sum()), name
            assert out[1] == max(int(x["nbytes"]) or 40 for x in vs), name
    assert seen == {OK, EINVAL, ECHANNEL, ELENGTH}


def test_create_refuses_what_the_mixed_decoder_refuses(emu):
    out = np.zeros(2, np.int32)
    v, b = views_of(view()), bounds()
    for desc, want in (((48000, 10000, 40), OK), ((8000, 7500, 1), OK), ((44100, 10000, 400), OK), ((48000, 5000, 40), EINVAL),
                       ((22050, 10000, 40), EINVAL), ((48000, 10000, 0), ELENGTH), ((48000, 10000, 401), ELENGTH)):
        d = descs_array([desc])
        assert emu.lc3emu_iv_check(P(d), 1, 8, P(v), 1, P(b), P(out)) == want, desc


def test_frames_per_workgroup_follow_the_lds_rule(emu):
    """256 lanes, halved down to 64 while 9824 + fpb * (192 + nbytes) + 8 bytes pass 64 KB"""
    for nb in range(1, 401):
        fpb = 256
        while fpb > 64 and 9824 + fpb * (192 + nb) + 8 > 65536:
            fpb //= 2
        assert emu.lc3emu_iv_fpb(nb) == fpb, nb
        assert emu.lc3emu_iv_lds(nb) == 9824 + fpb * (192 + nb) + 8 <= 65536, nb
    assert [emu.lc3emu_iv_fpb(nb) for nb in (1, 25, 26, 243, 244, 400)] == [256, 256, 128, 128, 64, 64]


def _plan(emu, descs, vs, fpb, max_nb):
    d = descs_array(descs)
    total = int(vs["n_frames"].astype(np.int64).sum())
    lanes = np.zeros((total + 1, 4), np.int64)
    wgs = np.zeros((total + len(vs) + 1, 5), np.int32)
    out = np.zeros(3, np.int32)
    rc = emu.lc3emu_iv_plan(P(d), len(descs), P(vs), len(vs), fpb, max_nb, P(lanes), total, P(wgs), len(wgs), P(out))
    assert rc == 0, rc
    return lanes[:total], wgs[: out[1]], int(out[0]), int(out[2])


@pytest.mark.parametrize("seed,fpb", [(1, 0), (2, 64), (3, 128), (4, 256), (5, 0), (6, 64)])
def test_every_frame_of_every_view_is_one_lane_of_one_uniform_workgroup(emu, seed, fpb):
    rng = np.random.default_rng(seed)
    descs = [(fs, us, int(rng.choice([20, 40, 57, 150]))) for fs, us in I.CONFIGS for _ in range(2)]
    n_views = int(rng.integers(1, 200))
    vs, expect, key_of_src = [], [], {}
    bo, fo = 12, 0
    for _ in range(n_views):
        ch = int(rng.integers(len(descs)))
        T = int(rng.choice([1, 1, 1, 2, 3, 7, 70, 300]))
        nbytes = int(rng.choice([0, 0, 1, 6, 7, 20, 57, 400]))
        nb = nbytes or descs[ch][2]
        bp, fp = int(rng.choice([0, nb, nb + 12, 412])), int(rng.choice([0, 1, 2, 9]))
        if bp < nb:
            bp = 0
        vs.append(view(channel=ch, n_frames=T, nbytes=nbytes, byte_off=bo, flag_off=fo, byte_pitch=bp, flag_pitch=fp))
        for t in range(T):
            src = bo + t * (bp or nb)
            expect.append((src, fo + t * (fp or 1)))
            key_of_src[src] = (descs[ch][0], descs[ch][1], nb)
        bo += T * (bp or nb) + int(rng.integers(0, 50))
        fo += T * (fp or 1) + int(rng.integers(0, 5))
    vs = views_of(*vs)
    max_nb = max(k[2] for k in key_of_src.values())
    lanes, wgs, n_buckets, used_fpb = _plan(emu, descs, vs, fpb, max_nb)
    assert used_fpb == (fpb or emu.lc3emu_iv_fpb(max_nb))
    assert sorted(map(tuple, lanes[:, 2:].tolist())) == sorted(expect)  # every (view, frame) once: the placements are all distinct
    assert len(set(expect)) == len(expect)
    # lanes of a workgroup: 0 .. frames - 1, in launch order; no workgroup is empty or over-full
    assert (wgs[:, 1] >= 1).all() and (wgs[:, 1] <= used_fpb).all() and int(wgs[:, 1].sum()) == len(expect)
    pos = 0
    for w, (bucket, nfr, nb, ne, fs_ind_ms) in enumerate(wgs.tolist()):
        rows = lanes[pos: pos + nfr]
        assert rows[:, 0].tolist() == [w] * nfr and rows[:, 1].tolist() == list(range(nfr))
        for src in rows[:, 2].tolist():  # uniform: every frame of the workgroup has the row's size and configuration
            fs, us, size = key_of_src[src]
            c = I.config(fs, us)
            assert (size, c.ne, c.fs_ind | (c.n_ms_10 << 8)) == (nb, ne, fs_ind_ms), (w, src)
        pos += nfr
    assert wgs[:, 0].tolist() == sorted(wgs[:, 0].tolist()) and len(set(wgs[:, 0].tolist())) == n_buckets
    # only a bucket's last workgroup may be partly filled
    for w in range(len(wgs) - 1):
        if wgs[w, 0] == wgs[w + 1, 0]:
            assert wgs[w, 1] == used_fpb


def test_the_lane_body_through_the_plan_over_a_tick_of_all_twelve_configurations(emu):
    rng = np.random.default_rng(20240)
    descs, vs, d_in, flags, n_out, frames = tick(rng)
    assert len(frames) > 2000 and {v["n_frames"] for v in vs} == {1, 3}
    want_status, want_info = expected_outputs(frames, n_out)
    assert len(set(want_status[[f[0] for f in frames]].tolist())) >= 8  # OK, flagged, side-information and arithmetic errors
    d = descs_array(descs)
    for use_flags in (True, False):
        if not use_flags:
            want_status, want_info = expected_outputs([(i, fs, us, fr, 0) for i, fs, us, fr, _ in frames], n_out)
        status = np.full(n_out, 0xCC, np.uint8)
        info = np.full((n_out, 32), 0x5A5A5A5A, np.uint32).view(np.int32)
        rc = emu.lc3emu_iv_run(P(d), len(descs), len(vs), P(vs), len(vs), P(d_in), d_in.size, P(flags) if use_flags else None, n_out, P(status), n_out,
                               P(info), n_out)
        assert rc == OK
        assert np.array_equal(status, want_status), np.nonzero(status != want_status)[0][:8]
        bad = np.nonzero((info != want_info).any(1))[0]
        assert not len(bad), (bad[:4], info[bad[0]].tolist(), want_info[bad[0]].tolist())
        assert not (want_status[[f[0] for f in frames]] == I.EMPTY).any()
    # status only, records only: the same values, the other array untouched; a refused call writes nothing
    status = np.full(n_out, 0xCC, np.uint8)
    assert emu.lc3emu_iv_run(P(d), len(descs), len(vs), P(vs), len(vs), P(d_in), d_in.size, None, 0, P(status), n_out, None, 0) == OK
    assert np.array_equal(status, want_status)
    status[:] = 0xCC
    assert emu.lc3emu_iv_run(P(d), len(descs), len(vs), P(vs), len(vs), P(d_in), int(vs["byte_off"].max()), None, 0, P(status), n_out, None, 0) == ELENGTH
    assert (status == 0xCC).all()


def test_the_check_and_the_plan_under_address_and_undefined_behaviour_sanitizers():
    """the stand-alone program (its own main, nothing preloaded, nothing loaded into Python) over the same extreme lists, as a child process"""
    src = os.path.join(EMU_DIR, "lc3_inspect_views_check_main.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe, case_file = os.path.join(tmp, "check_main"), os.path.join(tmp, "cases.bin")
        # (the runtimes linked statically: the program is whole, whatever else a machine loads into every process)
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                            "-static-libubsan", "-o", exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            if "sanitize" in r.stdout or "asan" in r.stdout or "ubsan" in r.stdout:
                pytest.skip("the compiler cannot link the sanitizer runtime: " + r.stdout.strip().splitlines()[-1])
            pytest.fail(r.stdout)
        todo = [c for c in cases() if c[1] is not None]
        rng = np.random.default_rng(9)
        for _ in range(20):  # random lists too, planned and walked whole
            vs = views_of(*[view(channel=int(rng.integers(12)), n_frames=int(rng.integers(1, 400)), nbytes=int(rng.choice([0, 1, 7, 400])),
                                 byte_off=int(rng.integers(0, 1000)), flag_off=int(rng.integers(0, 1000)), flag_pitch=int(rng.integers(0, 4)))
                            for _ in range(int(rng.integers(1, 60)))])
            todo.append(("random", vs, len(vs), bounds(in_bytes=1 << 20, n_flags=4096, n_status=4096, n_info=4096), 64, OK))
        blob = struct.pack("<i", len(todo))
        for name, vs, n, b, max_views, want in todo:
            blob += struct.pack("<i", len(DESCS)) + descs_array(DESCS).tobytes() + struct.pack("<ii", max_views, n)
            blob += (vs.tobytes() if n > 0 else b"") + b.tobytes() + struct.pack("<i", want)
        with open(case_file, "wb") as f:
            f.write(blob)
        r = subprocess.run([exe, case_file], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        words = r.stdout.split()
        assert words[0] == "ok" and int(words[1]) == len(todo) and int(words[2]) > 10000, r.stdout
