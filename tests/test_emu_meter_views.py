"""lc3gpu_measure_mixed_views on the CPU (no GPU needed): the check and row header the companion library runs on the host
(lc3-codec_amd/csrc/lc3_host_measure_views.h over lc3_host_inspect_views.h) through tests/emu/lc3_emu_meter_views.cpp -- every row of the
header's refusal table with its code, the first and the last sample and output index exactly and one beyond, max_views exactly and one more
--, and the kernel's lane body (lc3_dev_level.h) driven through the rows, wave by wave, the lanes folded in descending order, over the shapes
and the state scenarios of the GPU tests, bit for bit against the model (meter_lib).  The scenarios are written once, here, against a
`runner` (make, call, reset, close): this file gives them the emulator, tests/test_gpu_meter_views.py the device.  The same hostile lists go
through a stand-alone program built with -fsanitize=address,undefined (tests/emu/lc3_meter_views_check_main.cpp)."""
import ctypes
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import meter_lib as ML
from meter_lib import desc
from mix_lib import view, views_of

api = ML.api
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "liblc3emu_meter_views.so")

OK, EINVAL, ECHANNEL, ELENGTH = 0, -1, -2, -3
M31 = 2**31 - 1

# the channels of the refusal table
TABLE_DESCS = [desc(48000, 10000), desc(16000, 10000), desc(8000, 7500), desc(44100, 7500)]
C48, C16, C8S, C441S = range(4)  # nf 480, 160, 60, 360


def _build():
    csrc = os.path.join(ROOT, "lc3-codec_amd", "csrc")
    srcs = [os.path.join(EMU_DIR, "lc3_emu_meter_views.cpp")] + [os.path.join(csrc, f) for f in ("lc3_dev_level.h", "lc3_host_measure_views.h",
                                                                                               "lc3_host_inspect_views.h")]
    if not (os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in srcs)):
        tmp = LIB + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-strict-aliasing", "-Wno-unknown-pragmas", "-Wno-attributes", "-o", tmp,
                               srcs[0]])
        os.replace(tmp, LIB)
    L = ctypes.CDLL(LIB)
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    L.lc3emu_mt_new.argtypes = [vp, i, i, vp]
    L.lc3emu_mt_new.restype = vp
    L.lc3emu_mt_free.argtypes = [vp]
    L.lc3emu_mt_free.restype = None
    L.lc3emu_mt_reset.argtypes = [vp, vp, i]
    L.lc3emu_mt_state.argtypes = [vp, vp]
    L.lc3emu_mt_state.restype = None
    L.lc3emu_mt_check.argtypes = [vp, vp, i, vp]
    L.lc3emu_mt_run.argtypes = [vp, vp, i, vp, u64, vp, u64, vp, u64]
    L.lc3emu_mt_info.argtypes = [vp]
    L.lc3emu_mt_info.restype = None
    return L


@pytest.fixture(scope="module")
def emu():
    return _build()


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def descs_array(descs):
    return np.ascontiguousarray(np.array(descs, np.int64).astype(np.uint32).view(np.int32).reshape(-1, 6))


def emu_new(emu, descs, max_views):
    rc = np.zeros(1, np.int32)
    h = emu.lc3emu_mt_new(P(descs_array(descs)), len(descs), max_views, P(rc))
    return h, int(rc[0])


def aligned_levels(levels):
    """a copy of the records at a 16-byte aligned address"""
    raw = np.zeros(levels.nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    out = raw[off:off + levels.nbytes].view(api.LEVEL_DTYPE)
    out[:] = levels
    return out


class EmuRunner:
    """the scenarios' runner over the emulator"""

    def __init__(self, emu, descs, max_views):
        self.emu, self.n = emu, len(descs)
        self.h, rc = emu_new(emu, descs, max_views)
        assert rc == OK and self.h

    def call(self, views, pcm, active=None, levels=None, n_views=None, pcm_elems=None, n_active=None, n_levels=None, levels_shift=0):
        """-> (code, the whole of either output after the call); levels_shift: bytes the record array's address is off by"""
        a = None if active is None else np.array(active, np.uint8, copy=True)
        lv = None if levels is None else aligned_levels(levels)
        lp = None if lv is None else ctypes.c_void_p(lv.ctypes.data + levels_shift)
        pin = np.ascontiguousarray(pcm)
        vs = np.ascontiguousarray(views)
        rc = self.emu.lc3emu_mt_run(self.h, P(vs), len(vs) if n_views is None else n_views, P(pin), len(pin) if pcm_elems is None else pcm_elems, P(a),
                                    (0 if a is None else len(a)) if n_active is None else n_active, lp,
                                    (0 if lv is None else len(lv)) if n_levels is None else n_levels)
        return rc, a, lv

    def reset(self, channels=None):
        if channels is None:
            return self.emu.lc3emu_mt_reset(self.h, None, -1)
        ch = np.ascontiguousarray(np.asarray(channels, np.int32))
        return self.emu.lc3emu_mt_reset(self.h, P(ch), len(ch))

    def close(self):
        self.emu.lc3emu_mt_free(self.h)
        self.h = None


# three arrays far apart
BOUNDS = dict(pcm_base=0x10000000, pcm_elems=1 << 20, active_base=0x20000000, n_active=1 << 16, levels_base=0x30000000, n_levels=1 << 16, use_active=1,
              use_levels=1)
KEYS = ("pcm_base", "pcm_elems", "active_base", "n_active", "levels_base", "n_levels", "use_active", "use_levels")


def bounds(**over):
    b = dict(BOUNDS, **over)
    return np.array([b[k] for k in KEYS], np.uint64)


def cases():
    """(name, views, n_views, bounds, max_views, want) over TABLE_DESCS: the header's refusal table and the extremes.  views None is a null
    pointer."""
    C = []
    v1 = view(channel=C48, n_frames=3, pcm_off=10, flag_off=5)  # 1440 samples at 10, indices 5, 6, 7

    def add(name, want, vs=(v1,), n=None, max_views=64, null=False, **over):
        a = views_of(*vs)
        C.append((name, None if null else a, len(a) if n is None else n, bounds(**over), max_views, want))

    add("plain: three frames", OK)
    add("every channel once", OK, vs=[view(channel=c, pcm_off=1000 * c, flag_off=c) for c in range(4)])
    add("nothing at all", OK, vs=())
    add("nothing at all, null list and arrays", OK, vs=(), null=True, pcm_base=0, pcm_elems=0, use_active=0, use_levels=0)
    for ch in (-1, 4, M31):
        add("channel %d" % ch, ECHANNEL, vs=(view(channel=ch, n_frames=3),))
    add("a channel named twice", ECHANNEL, vs=(v1, view(channel=C48, n_frames=1, pcm_off=5000, flag_off=20)))
    add("a channel named twice, far apart", ECHANNEL, vs=(v1, view(channel=C16, pcm_off=5000, flag_off=20), view(channel=C48, pcm_off=8000, flag_off=30)))
    for n in (0, -1, -M31 - 1):
        add("n_frames %d" % n, ELENGTH, vs=(view(channel=C48, n_frames=n),))
    # more than 2^31 - 1 samples in one view: 480 * 4473925 = 2^31 + 352
    huge = dict(pcm_elems=1 << 40, n_active=1 << 40, n_levels=1 << 40, active_base=1 << 50, levels_base=1 << 60)
    add("2^31 - 1 samples or fewer", OK, vs=(view(channel=C48, n_frames=4473924),), **huge)
    add("more than 2^31 - 1 samples in a view", ELENGTH, vs=(view(channel=C48, n_frames=4473925),), **huge)
    add("2^31 - 1 frames", ELENGTH, vs=(view(channel=C8S, n_frames=M31),), **huge)
    # extents: the first and the last sample exactly, and one beyond
    last = 10 + 2 * 480 + 479
    add("the view ends at the end", OK, pcm_elems=last + 1)
    add("the view ends one beyond", ELENGTH, pcm_elems=last)
    add("the view begins at the first sample", OK, vs=(view(channel=C48, n_frames=3, pcm_off=0, flag_off=5),), pcm_elems=1440)
    add("pcm_off at the end", ELENGTH, vs=(view(channel=C48, n_frames=3, pcm_off=1 << 20),))
    sp = view(channel=C16, n_frames=3, pcm_off=7, pcm_stride=8, pcm_pitch=4000)
    add("a strided pitched view ends at the end", OK, vs=(sp,), pcm_elems=7 + 2 * 4000 + 159 * 8 + 1)
    add("a strided pitched view ends one beyond", ELENGTH, vs=(sp,), pcm_elems=7 + 2 * 4000 + 159 * 8)
    add("the second view is the bad one", ELENGTH, vs=(v1, view(channel=C16, pcm_off=(1 << 20) - 158)))
    # output indices: 5, 6, 7 and, pitched, 5, 8, 11
    add("the last record is the last", OK, n_levels=8)
    add("the last record lies one beyond", ELENGTH, n_levels=7)
    add("the last byte is the last", OK, n_active=8)
    add("the last byte lies one beyond", ELENGTH, n_active=7)
    add("an output that is not given is checked against nothing", OK, n_levels=0, use_levels=0)
    add("an activity array that is not given is checked against nothing", OK, n_active=0, use_active=0)
    vp3 = view(channel=C48, n_frames=3, pcm_off=10, flag_off=5, flag_pitch=3)
    add("a flag pitch of 3 ends at the end", OK, vs=(vp3,), n_levels=12, n_active=12)
    add("a flag pitch of 3 ends one beyond in the records", ELENGTH, vs=(vp3,), n_levels=11, n_active=12)
    add("a flag pitch of 3 ends one beyond in the bytes", ELENGTH, vs=(vp3,), n_levels=12, n_active=11)
    add("flag_off at the end", ELENGTH, vs=(view(channel=C48, flag_off=1 << 16),))
    # the longest view at a pitch of 2^31 - 1, offsets near 2^62 and 2^63
    T = M31 // 60
    vl = view(channel=C8S, n_frames=T, pcm_stride=8, pcm_pitch=M31, flag_pitch=M31)
    span, fspan = (T - 1) * M31 + 59 * 8, (T - 1) * M31
    far = dict(pcm_base=4, active_base=1 << 62, levels_base=(1 << 63) + (1 << 62))
    add("the longest view at pitches of 2^31 - 1 fits", OK, vs=(vl,), pcm_elems=span + 1, n_active=fspan + 1, n_levels=min(fspan + 1, (1 << 57)), use_levels=0, **far)
    add("the longest view: one sample short", ELENGTH, vs=(vl,), pcm_elems=span, n_active=fspan + 1, use_levels=0, **far)
    add("the longest view: one byte short", ELENGTH, vs=(vl,), pcm_elems=span + 1, n_active=fspan, use_levels=0, **far)
    s8 = view(channel=C8S, pcm_off=1 << 62)
    add("pcm_off 2^62 inside", OK, vs=(s8,), pcm_elems=(1 << 62) + 60, pcm_base=4, active_base=(1 << 63) + (1 << 62), use_levels=0)
    add("pcm_off 2^62: one sample short", ELENGTH, vs=(s8,), pcm_elems=(1 << 62) + 59, pcm_base=4, active_base=(1 << 63) + (1 << 62), use_levels=0)
    f62 = view(channel=C8S, flag_off=2**63 - 1)
    add("flag_off 2^63 - 1 inside", OK, vs=(f62,), n_active=2**63, active_base=1 << 30, pcm_base=4096, pcm_elems=60, use_levels=0)
    add("flag_off 2^63 - 1: one byte short", ELENGTH, vs=(f62,), n_active=2**63 - 1, active_base=1 << 30, pcm_base=4096, pcm_elems=60, use_levels=0)
    add("a negative pcm_off", EINVAL, vs=(view(channel=C48, n_frames=3, pcm_off=-2),))
    add("the most negative pcm_off", EINVAL, vs=(view(channel=C48, n_frames=3, pcm_off=-2**63),))
    add("a negative flag_off", EINVAL, vs=(view(channel=C48, n_frames=3, flag_off=-1),))
    add("the most negative flag_off", EINVAL, vs=(view(channel=C48, n_frames=3, flag_off=-2**63),))
    # max_views exactly, and one more
    two = (v1, view(channel=C16, pcm_off=3000, flag_off=20))
    add("as many views as max_views", OK, vs=two, max_views=2)
    add("one view more than max_views", ELENGTH, vs=two, max_views=1)
    # placement
    for st, want in ((0, EINVAL), (-1, EINVAL), (9, EINVAL), (M31, EINVAL), (1, OK), (2, OK), (8, OK)):
        add("pcm_stride %d" % st, want, vs=(view(channel=C48, n_frames=3, pcm_stride=st),))
    add("a pitch below the frame", EINVAL, vs=(view(channel=C48, n_frames=3, pcm_pitch=478),))
    add("a pitch of the frame", OK, vs=(view(channel=C48, n_frames=3, pcm_pitch=480),))
    add("a pitch below the strided frame", EINVAL, vs=(view(channel=C48, n_frames=3, pcm_stride=2, pcm_pitch=959),))
    add("a pitch of the strided frame", OK, vs=(view(channel=C48, n_frames=3, pcm_stride=2, pcm_pitch=960),))
    add("a negative pitch", EINVAL, vs=(view(channel=C48, n_frames=3, pcm_pitch=-480),))
    add("a negative flag pitch", EINVAL, vs=(view(channel=C48, n_frames=3, flag_pitch=-1),))
    for k in range(3):
        add("reserved[%d]" % k, EINVAL, vs=(view(channel=C48, n_frames=3, reserved=tuple(int(j == k) for j in range(3))),))
    add("the fields the call does not read", OK, vs=(view(channel=C48, n_frames=3, nbytes=-5, byte_off=-9, byte_pitch=-1),))
    # alignment
    add("planar with an odd pcm_off", EINVAL, vs=(view(channel=C48, n_frames=3, pcm_off=11),))
    add("planar with an odd pitch", EINVAL, vs=(view(channel=C48, n_frames=3, pcm_pitch=481),))
    add("strided with an odd pcm_off and an odd pitch", OK, vs=(view(channel=C48, n_frames=3, pcm_off=11, pcm_stride=2, pcm_pitch=961),))
    for mis in (1, 2, 3):
        add("planar, base off by %d" % mis, EINVAL, pcm_base=BOUNDS["pcm_base"] + mis)
        add("strided, base off by %d" % mis, OK if mis == 2 else EINVAL, vs=(view(channel=C48, n_frames=3, pcm_stride=2),), pcm_base=BOUNDS["pcm_base"] + mis)
    for mis in (1, 2, 4, 8, 12):
        add("records off by %d" % mis, EINVAL, levels_base=BOUNDS["levels_base"] + mis)
    add("records off by 16", OK, levels_base=BOUNDS["levels_base"] + 16)
    add("an activity array at an odd address", OK, active_base=BOUNDS["active_base"] + 1)
    add("both outputs null", EINVAL, use_active=0, use_levels=0)
    # the address ranges, at either end; touching is no overlap
    I0, IL = BOUNDS["pcm_base"], 2 * BOUNDS["pcm_elems"]
    add("the records end where the PCM begins", OK, levels_base=I0 - 4096, n_levels=128)
    add("the last record's last byte is the PCM's first", EINVAL, levels_base=I0 - 4096 + 16, n_levels=128)
    add("the records begin where the PCM ends", OK, levels_base=I0 + IL)
    add("the records begin in the PCM's last sample", EINVAL, levels_base=I0 + IL - 16)
    add("the bytes end where the PCM begins", OK, active_base=I0 - 100, n_active=100)
    add("the last byte is the PCM's first", EINVAL, active_base=I0 - 99, n_active=100)
    add("the bytes begin where the PCM ends", OK, active_base=I0 + IL)
    add("the bytes begin at the PCM's last byte", EINVAL, active_base=I0 + IL - 1)
    add("the bytes inside the PCM, and not given", OK, active_base=I0 + 64, use_active=0)
    add("the bytes inside the records", EINVAL, active_base=BOUNDS["levels_base"] + 64, n_active=8)
    add("the bytes end where the records begin", OK, active_base=BOUNDS["levels_base"] - 8, n_active=8)
    add("the records are the PCM", EINVAL, levels_base=I0)
    add("an array that ends at 2^64", OK, levels_base=2**64 - 4096, n_levels=128)
    add("an array whose length passes 2^64 overlaps what lies behind it", EINVAL, pcm_base=2**63, levels_base=4096, n_levels=2**59 + 8, use_active=0)
    # null pointers and counts
    add("null views", EINVAL, null=True)
    add("null d_pcm", EINVAL, pcm_base=0)
    add("n_views < 0", EINVAL, n=-1)
    return C


def test_every_refusal_and_every_extreme_has_its_code(emu):
    seen = set()
    for name, vs, n, b, max_views, want in cases():
        h, rc = emu_new(emu, TABLE_DESCS, max_views)
        assert rc == OK
        emu.lc3emu_mt_reset(h, P(np.array([C16], np.int32)), 1)
        before = np.zeros((4, 4), np.int32)
        emu.lc3emu_mt_state(h, P(before))
        for _ in range(2):  # (a check leaves nothing behind that the next one meets: the named-twice marks least of all)
            rc = emu.lc3emu_mt_check(h, P(vs), n, P(b))
            assert rc == want, (name, rc, want)
        after = np.zeros((4, 4), np.int32)
        emu.lc3emu_mt_state(h, P(after))
        assert np.array_equal(before, after), name  # state and pending resets as they were
        emu.lc3emu_mt_free(h)
        seen.add(rc)
    assert seen == {OK, EINVAL, ECHANNEL, ELENGTH}


def test_create_takes_the_twelve_configurations_and_holds_every_field_to_its_range(emu):
    def new(d, mv=4):
        h, rc = emu_new(emu, [d], mv)
        if h:
            emu.lc3emu_mt_free(h)
        return rc

    for fs, us in ML.CONFIGS:
        assert new(desc(fs, us)) == OK
    for d in (desc(22050, 10000), desc(48000, 5000), desc(0, 10000), desc(48000, 0), desc(-8000, 7500)):
        assert new(d) == EINVAL, d
    for lo_hi in ((0, 0), (32768, 32768), (0, 32768)):
        assert new(desc(48000, 10000, attack=lo_hi[0], release=lo_hi[1])) == OK
    for bad in (-1, 32769, M31, -M31 - 1):
        assert new(desc(48000, 10000, attack=bad)) == EINVAL and new(desc(48000, 10000, release=bad)) == EINVAL
    assert new(desc(48000, 10000, threshold=0)) == OK and new(desc(48000, 10000, threshold=1 << 30)) == OK
    assert new(desc(48000, 10000, threshold=(1 << 30) + 1)) == EINVAL and new(desc(48000, 10000, threshold=2**32 - 1)) == EINVAL
    assert new(desc(48000, 10000, hang=0)) == OK and new(desc(48000, 10000, hang=65535)) == OK
    assert new(desc(48000, 10000, hang=-1)) == EINVAL and new(desc(48000, 10000, hang=65536)) == EINVAL
    assert new(desc(48000, 10000), mv=0) == EINVAL and new(desc(48000, 10000), mv=-1) == EINVAL
    rc = np.zeros(1, np.int32)
    assert not emu.lc3emu_mt_new(None, 1, 4, P(rc)) and rc[0] == EINVAL
    assert not emu.lc3emu_mt_new(P(descs_array([desc(8000, 7500)])), 0, 4, P(rc)) and rc[0] == EINVAL
    h, rc = emu_new(emu, [desc(8000, 7500), desc(48000, 10000, hang=70000)], 4)  # the second descriptor is the bad one
    assert not h and rc == EINVAL
    info = np.zeros(5, np.int32)
    emu.lc3emu_mt_info(P(info))
    assert info.tolist() == [4, 256, 64, 16, 64]


# ---- the scenarios: written against a runner, run here on the emulator and in tests/test_gpu_meter_views.py on the device ------------------
def assert_outputs(got_a, got_lv, want_a, want_lv, what):
    """the WHOLE of either output: the frames' own bytes and records, and the sentinels between and around them"""
    if want_a is not None:
        bad = np.flatnonzero(got_a != want_a)
        assert bad.size == 0, "%s: activity byte %d is %d, the model's %d" % (what, bad[0], got_a[bad[0]], want_a[bad[0]])
    if want_lv is not None:
        bad = np.flatnonzero(got_lv != want_lv)
        assert bad.size == 0, "%s: record %d is %s, the model's %s" % (what, bad[0], got_lv[bad[0]], want_lv[bad[0]])


ALL_DESCS = [desc(fs, us, attack=(8192, 32768, 20000)[k % 3], release=(1024, 4096, 0)[k % 3], threshold=(1 << 12, 1 << 22, 40000)[k % 3], hang=k % 4)
             for k, (fs, us) in enumerate(ML.CONFIGS)]


def shape_ticks():
    """name -> Tick.  The twelve configurations x strides 1, 2, 8 x one and three frames x compact and padded pitches x flag_pitch 0 and 3:
    nf = 60 is 30 words, less than a wave; nf = 480 is 240 words, a ragged fourth pass.  Twelve views a call: three workgroups."""
    ticks = {}
    for k, (stride, T, gap, fp) in enumerate((s, T, g, fp) for s in (1, 2, 8) for T in (1, 3) for g in (0, 38) for fp in (0, 3)):
        rng = np.random.default_rng(100 + k)
        name = "stride %d, %d frame%s, %s, flag_pitch %d" % (stride, T, "s" * (T > 1), "padded" if gap else "compact", fp)
        ticks[name] = ML.make_tick(ALL_DESCS, [(ch, T, stride, gap, fp) for ch in range(12)], rng)
    return ticks


SHAPE_NAMES = list(shape_ticks())


def scenario_shape(make, t, what):
    """two calls of the same tick: the second continues the first's states.  Only bytes, only records, both."""
    for outs in ("both", "active", "levels"):
        run, mod = make(t.descs, t.max_views), ML.Model(t.descs)
        a = t.active if outs != "levels" else None
        lv = t.levels if outs != "active" else None
        for k in range(2):
            want_a, want_lv = mod.call(t.views, t.pcm, a, lv)
            rc, got_a, got_lv = run.call(t.views, t.pcm, a, lv)
            assert rc == OK, (what, outs, rc)
            assert_outputs(got_a, got_lv, want_a, want_lv, "%s, %s, call %d" % (what, outs, k))
            if want_lv is not None:
                assert (want_lv["reserved0"] == ML.LEVEL_SENTINEL).sum() >= 1 and (want_lv["reserved0"] == 0).sum() == sum(int(v["n_frames"]) for v in t.views)
        run.close()


def scenario_views_per_call(make):
    """1, 3, 4, 5 and 9 views a call: below, at and above a workgroup's four waves"""
    for n in (1, 3, 4, 5, 9):
        rng = np.random.default_rng(200 + n)
        t = ML.make_tick(ALL_DESCS, [(ch, 1 + ch % 2, (1, 2, 8)[ch % 3], (0, 6)[ch % 2], (0, 3)[ch % 2]) for ch in rng.permutation(12)[:n]], rng)
        run, mod = make(t.descs, t.max_views), ML.Model(t.descs)
        want_a, want_lv = mod.call(t.views, t.pcm, t.active, t.levels)
        rc, got_a, got_lv = run.call(t.views, t.pcm, t.active, t.levels)
        assert rc == OK
        assert_outputs(got_a, got_lv, want_a, want_lv, "%d views" % n)
        run.close()


def scenario_split_invariance(make):
    """six frames in one view; as 2 + 4 over two calls; as six calls: the records are identical, at either stride"""
    for stride, ch in ((1, 9), (2, 3), (1, 0)):  # (nf 480, 120 and 60; channels whose envelope rises and falls)
        rng = np.random.default_rng(300 + ch)
        nf = ML.nf_of(*ALL_DESCS[ch][:2])
        x = np.concatenate([rng.integers(-a, a + 1, nf) for a in (20000, 50, 0, 32767, 3, 900)])
        t = ML.make_tick(ALL_DESCS, [(ch, 6, stride, 0, 0)], rng, data={ch: x})
        v = t.views[0]
        pitch = nf * stride
        want_a, want_lv = ML.Model(t.descs).call(t.views, t.pcm, t.active, t.levels)
        assert len(set(int(e) for e in want_lv["env"][int(v["flag_off"]):int(v["flag_off"]) + 6])) == 6  # (the recurrence matters)
        for split in ((6,), (2, 4), (1, 1, 1, 1, 1, 1)):
            run = make(t.descs, t.max_views)
            a, lv, done = t.active, t.levels, 0
            for n in split:
                part = view(channel=ch, n_frames=n, pcm_off=int(v["pcm_off"]) + done * pitch, pcm_stride=stride, flag_off=int(v["flag_off"]) + done)
                rc, a, lv = run.call(part, t.pcm, a, lv)
                assert rc == OK
                done += n
            assert_outputs(a, lv, want_a, want_lv, "split %s, stride %d" % (split, stride))
            run.close()


def scenario_state(make):
    """channels not listed keep their state; reset and reset_channels; refused calls leave state and pending resets as they were"""
    rng = np.random.default_rng(41)
    descs = [desc(16000, 10000, threshold=1 << 14, hang=3), desc(48000, 7500, threshold=1 << 14, hang=1), desc(8000, 10000, threshold=1 << 14, hang=2)]
    t = ML.make_tick(descs, [(0, 2, 1, 0, 0), (1, 1, 2, 6, 0), (2, 2, 8, 0, 3)], rng, data={c: rng.integers(-9000, 9000, 2000) for c in range(3)}, shuffle=False)
    quiet = (t.pcm // 64).astype(np.int16)
    run, mod = make(descs, t.max_views), ML.Model(descs)

    def both(views, pcm, what, **over):
        want_a, want_lv = mod.call(views, pcm, t.active, t.levels)
        rc, a, lv = run.call(views, pcm, t.active, t.levels, **over)
        assert rc == OK, (what, rc)
        assert_outputs(a, lv, want_a, want_lv, what)

    def refused(want, views, what, **over):
        rc, a, lv = run.call(views, t.pcm, t.active, t.levels, **over)
        assert rc == want, (what, rc)
        assert np.array_equal(a, t.active) and np.array_equal(lv, t.levels), what  # nothing written

    both(t.views, t.pcm, "all three")
    both(t.views[1:2], quiet, "only channel 1: the others keep their state")
    both(t.views, quiet, "all three again")
    assert run.reset([1]) == OK
    mod.reset([1])
    # refused calls between the reset and the next good call: the pending reset stays pending, no channel advances
    twice = views_of(t.views[0:1], t.views[1:2], view(channel=0, pcm_off=0, flag_off=0))
    refused(ECHANNEL, twice, "a channel named twice")
    refused(ELENGTH, t.views, "a record out of extent", n_levels=int(max(v["flag_off"] + (v["n_frames"] - 1) * (v["flag_pitch"] or 1) for v in t.views)))
    refused(EINVAL, t.views, "misaligned records", levels_shift=8)
    both(t.views, t.pcm, "after reset_channels([1]) and three refused calls")
    assert run.reset([0, 3]) == ECHANNEL and run.reset([-1]) == ECHANNEL  # and then none is reset
    both(t.views, quiet, "after a refused reset_channels")
    assert run.reset() == OK
    mod.reset()
    both(t.views[::-1], t.pcm, "after reset, the views in another order")
    assert run.reset([]) == OK
    both(t.views, quiet, "after an empty reset_channels")
    run.close()


def scenario_worst_case(make):
    """all at nf = 480 and nf = 60: all -32768 (sum_sq = nf * 2^30, n_clipped = nf); alternating +32767 / -32768 (n_cross = nf or nf - 1, by
    the sign of last); attack 32768 from env 0 to 2^30 and release 32768 back to 0"""
    for fs, us, nf in ((48000, 10000, 480), (8000, 7500, 60)):
        for stride in (1, 2):
            descs = [desc(fs, us, attack=32768, release=32768, threshold=1 << 30, hang=1) for _ in range(3)]
            rng = np.random.default_rng(nf + stride)
            alt = np.tile([32767, -32768], nf)  # two frames; the second starts behind a negative sample
            data = {0: np.concatenate([np.full(nf, -32768), np.zeros(nf)]), 1: alt, 2: -alt - 1}
            t = ML.make_tick(descs, [(ch, 2, stride, 0, 0) for ch in range(3)], rng, data=data, shuffle=False)
            run, mod = make(descs, t.max_views), ML.Model(descs)
            want_a, want_lv = mod.call(t.views, t.pcm, t.active, t.levels)
            f = [int(v["flag_off"]) for v in t.views]
            r = want_lv[f[0]]
            assert r["sum_sq"] == nf << 30 and r["n_clipped"] == nf and r["env"] == 1 << 30 and r["sum"] == -32768 * nf and r["active"] == 1 and r["n_cross"] == 1
            r = want_lv[f[0] + 1]
            assert r["sum_sq"] == 0 and r["env"] == 0 and r["active"] == 1 and r["hang"] == 0 and r["n_cross"] == 1
            # +32767 first behind last = 0: no change into sample 0; then behind -32768: nf changes
            assert want_lv[f[1]]["n_cross"] == nf - 1 and want_lv[f[1] + 1]["n_cross"] == nf and want_lv[f[1]]["n_clipped"] == nf
            # -32768 first behind last = 0: nf changes; then behind +32767: nf again
            assert want_lv[f[2]]["n_cross"] == nf and want_lv[f[2] + 1]["n_cross"] == nf
            assert want_lv[f[1]]["sum_sq"] == (nf // 2) * (32767**2 + 32768**2)
            rc, a, lv = run.call(t.views, t.pcm, t.active, t.levels)
            assert rc == OK
            assert_outputs(a, lv, want_a, want_lv, "worst cases at nf %d, stride %d" % (nf, stride))
            run.close()


def scenario_gate(make):
    """two loud frames, then hang_frames + 2 silent ones, hang_frames in {0, 1, 3}: the sequence of active and hang"""
    for hang in (0, 1, 3):
        descs = [desc(16000, 10000, attack=32768, release=32768, threshold=1000, hang=hang)]
        T = hang + 4
        x = np.concatenate([np.tile([4000, -4000], 160), np.zeros(160 * (hang + 2))])
        t = ML.make_tick(descs, [(0, T, 1, 0, 0)], np.random.default_rng(hang), data={0: x})
        run = make(descs, 1)
        rc, a, lv = run.call(t.views, t.pcm, t.active, t.levels)
        assert rc == OK
        f = int(t.views[0]["flag_off"])
        assert lv["active"][f:f + T].tolist() == [1, 1] + [1] * hang + [0, 0]
        assert lv["hang"][f:f + T].tolist() == [hang, hang] + list(range(hang - 1, -1, -1)) + [0, 0]
        assert a[f:f + T].tolist() == lv["active"][f:f + T].tolist()
        want_a, want_lv = ML.Model(descs).call(t.views, t.pcm, t.active, t.levels)
        assert_outputs(a, lv, want_a, want_lv, "gate, hang_frames %d" % hang)
        run.close()


# ---- the scenarios on the emulator -----------------------------------------------------------------------------------------------------------
@pytest.fixture()
def make(emu):
    return lambda descs, max_views: EmuRunner(emu, descs, max_views)


@pytest.fixture(scope="module")
def ticks():
    return shape_ticks()


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_the_lane_body_through_the_rows_is_the_model_bit_for_bit(make, ticks, name):
    scenario_shape(make, ticks[name], name)


def test_the_shapes_are_the_ones_the_contract_names(ticks):
    assert len(ticks) == 3 * 2 * 2 * 2
    nfs = set()
    for t in ticks.values():
        assert sorted(int(v["channel"]) for v in t.views) == list(range(12))
        nfs |= {ML.nf_of(*t.descs[int(v["channel"])][:2]) for v in t.views}
    assert {60, 480} <= nfs and len(ML.CONFIGS) == 12


def test_views_per_call_below_at_and_above_a_workgroup(make):
    scenario_views_per_call(make)


def test_split_invariance(make):
    scenario_split_invariance(make)


def test_state_resets_and_refused_calls(make):
    scenario_state(make)


def test_worst_case_inputs_do_not_wrap(make):
    scenario_worst_case(make)


def test_the_gate_and_its_hang_over(make):
    scenario_gate(make)


def test_the_envelope_stays_between_env0_and_ms():
    """the header's bounds in Python integers over random and corner triples (a smaller run of the two million of the contract)"""
    rng = np.random.default_rng(6)
    corners = [0, 1, 2, (1 << 30) - 1, 1 << 30]
    triples = [(a, b, k) for a in corners for b in corners for k in (0, 1, 16384, 32767, 32768)]
    triples += [(int(a), int(b), int(k)) for a, b, k in zip(rng.integers(0, (1 << 30) + 1, 20000), rng.integers(0, (1 << 30) + 1, 20000), rng.integers(0, 32769, 20000))]
    for env0, ms, k in triples:
        d = ms - env0
        env = env0 + ((d * k + 16384) >> 15)
        assert min(env0, ms) <= env <= max(env0, ms) and abs(d * k) <= 1 << 45
        if k == 32768:
            assert env == ms
        if k == 0:
            assert env == env0


def test_the_check_and_the_row_builder_under_address_and_undefined_behaviour_sanitizers():
    """the stand-alone program (its own main, nothing preloaded, nothing loaded into Python) over the same hostile lists and the shapes, as
    a child process"""
    src = os.path.join(EMU_DIR, "lc3_meter_views_check_main.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe, case_file = os.path.join(tmp, "check_main"), os.path.join(tmp, "cases.bin")
        # (the runtimes linked statically: the program is whole, whatever else a machine loads into every process)
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                            "-static-libubsan", "-Wno-unknown-pragmas", "-o", exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            if "sanitize" in r.stdout or "asan" in r.stdout or "ubsan" in r.stdout:
                pytest.skip("the compiler cannot link the sanitizer runtime: " + r.stdout.strip().splitlines()[-1])
            pytest.fail(r.stdout)
        todo = [(TABLE_DESCS,) + c[1:] for c in cases() if c[1] is not None]  # (the file has no null pointers)
        for t in shape_ticks().values():
            todo.append((t.descs, t.views, len(t.views), bounds(pcm_elems=len(t.pcm), n_active=len(t.active), n_levels=len(t.levels)), t.max_views, OK))
        blob = struct.pack("<i", len(todo))
        for descs, vs, n, b, max_views, want in todo:
            blob += struct.pack("<i", len(descs)) + descs_array(descs).tobytes() + struct.pack("<ii", max_views, n)
            blob += vs[:n].tobytes() if n > 0 else b""
            blob += b.tobytes() + struct.pack("<i", want)
        with open(case_file, "wb") as f:
            f.write(blob)
        r = subprocess.run([exe, case_file], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        words = r.stdout.split()
        assert words[0] == "ok" and int(words[1]) == len(todo) and int(words[2]) > 500, r.stdout
