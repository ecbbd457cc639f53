"""lc3gpu_analyze_mixed_views on the CPU (no GPU needed): the check header the companion library runs on the host
(lc3-codec_amd/csrc/lc3_host_analyze_views.h over lc3_host_inspect_views.h) through tests/emu/lc3_emu_analyze_views.cpp -- every refusal of
the header's table with its code, offsets near 2^62 and 2^63, a pitch of 2^31 - 1 with 2^31 - 1 frames, the last element of each of the
five arrays and one further, the overlap refusals, max_frames exactly and one more, each misalignment --, and the kernel's lane body
(lc3_analyze_frame) driven through the plan over the corpus of all 12 configurations against the oracle's stage chain: spectrum rows bit
for bit, band and total energies bit for bit against the same formulas evaluated sequentially in float32.  The same extreme lists go
through a stand-alone program built with -fsanitize=address,undefined (tests/emu/lc3_analyze_views_check_main.cpp)."""
import ctypes
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import analyze_views_lib as A
import inspect_lib as I
from inspect_views_lib import view, views_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "liblc3emu_analyze_views.so")

OK, EINVAL, ECHANNEL, ELENGTH = 0, -1, -2, -3
DESCS = [(fs, us, 40) for fs, us in I.CONFIGS]
M31 = 2**31 - 1


def _build():
    srcs = [os.path.join(EMU_DIR, "lc3_emu_analyze_views.cpp"), os.path.join(EMU_DIR, "lc3_emu.cpp"), os.path.join(ROOT, "tables", "lc3_tables.h"),
            os.path.join(ROOT, "include", "lc3gpu.h")]
    csrc = os.path.join(ROOT, "lc3-codec_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not (os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in srcs)):
        tmp = LIB + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-strict-aliasing",
                               "-Wno-unknown-pragmas", "-Wno-attributes", "-o", tmp, srcs[0], "-lpthread"])
        os.replace(tmp, LIB)
    L = ctypes.CDLL(LIB)
    L.lc3emu_av_lds.restype = ctypes.c_longlong
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    L.lc3emu_av_check.argtypes = [vp, i, i, i, vp, i, vp, vp]
    L.lc3emu_av_run.argtypes = [vp, i, i, i, vp, i, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64]
    return L


@pytest.fixture(scope="module")
def emu():
    return _build()


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def descs_array(descs):
    return np.ascontiguousarray(np.array(descs, np.int32).reshape(-1, 3))


# five arrays far apart: in, flags, energy, bands, spec
BOUNDS = dict(in_base=0x10000000, in_bytes=1 << 20, flags_base=0x20000000, n_flags=1 << 16, energy_base=0x30000000, n_energy=1 << 16,
              bands_base=0x40000000, n_bands=1 << 16, spec_base=0x50000000, n_spec=1 << 16)
KEYS = ("in_base", "in_bytes", "flags_base", "n_flags", "energy_base", "n_energy", "bands_base", "n_bands", "spec_base", "n_spec")
ONLY_ENERGY = dict(bands_base=0, n_bands=0, spec_base=0, n_spec=0)


def bounds(**over):
    b = dict(BOUNDS, **over)
    return np.array([b[k] for k in KEYS], np.uint64)


def cases():
    """(name, views or None, n_views, bounds, max_views, max_frames, want): the header's refusal table and the extremes"""
    C = []

    def add(name, vs, want, n_views=None, max_views=64, max_frames=M31, **over):
        C.append((name, vs, len(vs) if n_views is None else n_views, bounds(**over), max_views, max_frames, want))

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
    # max_frames exactly, and one more
    add("as many frames as max_frames", views_of(one, view(n_frames=3)), OK, max_frames=7)
    add("one frame more than max_frames", views_of(one, view(n_frames=3)), ELENGTH, max_frames=6)
    add("one view beyond max_frames", views_of(view(n_frames=2)), ELENGTH, max_frames=1)
    add("one frame, max_frames 1", views_of(view()), OK, max_frames=1)
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
    add("all three outputs NULL", views_of(one), EINVAL, energy_base=0, **ONLY_ENERGY)
    add("all three outputs NULL, no views", views_of(), EINVAL, energy_base=0, **ONLY_ENERGY)
    add("energy only", views_of(one), OK, **ONLY_ENERGY)
    add("bands only", views_of(one), OK, energy_base=0, n_energy=0, spec_base=0, n_spec=0)
    add("spectra only", views_of(one), OK, energy_base=0, n_energy=0, bands_base=0, n_bands=0)
    add("no flags", views_of(one), OK, flags_base=0, n_flags=0)
    add("null views", None, EINVAL, n_views=1)
    add("n_views < 0", views_of(one), EINVAL, n_views=-1)
    add("null d_in", views_of(one), EINVAL, in_base=0)
    # each misalignment
    for mis in (1, 2, 3):
        add("d_energy off by %d" % mis, views_of(one), EINVAL, energy_base=BOUNDS["energy_base"] + mis)
        add("d_bands off by %d" % mis, views_of(one), EINVAL, bands_base=BOUNDS["bands_base"] + mis)
    for mis in (1, 2, 3, 4, 8, 12, 15):
        add("d_spec off by %d" % mis, views_of(one), EINVAL, spec_base=BOUNDS["spec_base"] + mis)
    add("d_energy and d_bands 4-byte aligned, d_spec 16-byte aligned", views_of(one), OK, energy_base=BOUNDS["energy_base"] + 4,
        bands_base=BOUNDS["bands_base"] + 12, spec_base=BOUNDS["spec_base"] + 16)
    # exactly at each array's end, and one element further
    add("bytes end at the end", views_of(view(n_frames=3, byte_off=12, byte_pitch=412)), OK, in_bytes=12 + 2 * 412 + 40)
    add("bytes end one past", views_of(view(n_frames=3, byte_off=12, byte_pitch=412)), ELENGTH, in_bytes=12 + 2 * 412 + 39)
    add("byte_off at the end", views_of(view(byte_off=1 << 20)), ELENGTH)
    for arr in ("n_flags", "n_energy", "n_bands", "n_spec"):
        v = views_of(view(n_frames=3, flag_off=7, flag_pitch=5))
        add("%s: the last index is the last element" % arr, v, OK, **{arr: 18})
        add("%s: one further" % arr, v, ELENGTH, **{arr: 17})
        add("%s: flag_off at the end" % arr, views_of(view(flag_off=18)), ELENGTH, **{arr: 18})
    add("flags not given: n_flags is not looked at", views_of(view(n_frames=3, flag_off=7, flag_pitch=5)), OK, flags_base=0, n_flags=1)
    add("energy not given: n_energy is not looked at", views_of(view(flag_off=7)), OK, energy_base=0, n_energy=1)
    add("bands not given: n_bands is not looked at", views_of(view(flag_off=7)), OK, bands_base=0, n_bands=1)
    add("spectra not given: n_spec is not looked at", views_of(view(flag_off=7)), OK, spec_base=0, n_spec=1)
    add("the second view is the bad one", views_of(one, view(n_frames=3, flag_off=(1 << 16) - 2)), ELENGTH)
    # frame counts
    big = dict(in_base=4096, in_bytes=1 << 40, flags_base=0, n_flags=0, energy_base=1 << 62, n_energy=1 << 40, **ONLY_ENERGY)
    add("2^31 - 1 frames", views_of(view(n_frames=M31, nbytes=1)), OK, **big)
    add("2^31 - 1 frames, max_frames one less", views_of(view(n_frames=M31, nbytes=1)), ELENGTH, max_frames=M31 - 1, **big)
    add("2^31 frames in two views", views_of(view(n_frames=M31, nbytes=1), view(n_frames=1, nbytes=1)), ELENGTH, **big)
    add("2^32 - 2 frames in two views", views_of(view(n_frames=M31, nbytes=1), view(n_frames=M31, nbytes=1)), ELENGTH, **big)
    # a pitch of 2^31 - 1 with 2^31 - 1 frames: the span is (2^31 - 2) * (2^31 - 1) + the last element
    span = (M31 - 1) * M31
    far = dict(in_base=4096, flags_base=0, n_flags=0, energy_base=1 << 63, **ONLY_ENERGY)
    v = views_of(view(n_frames=M31, byte_pitch=M31, flag_pitch=M31))
    add("the longest view fits", v, OK, in_bytes=span + 40, n_energy=span + 1, **far)
    add("the longest view: one byte short", v, ELENGTH, in_bytes=span + 39, n_energy=span + 1, **far)
    add("the longest view: one float short", v, ELENGTH, in_bytes=span + 40, n_energy=span, **far)
    add("the longest view from 2^62 on", views_of(view(n_frames=M31, byte_pitch=M31, flag_pitch=M31, byte_off=1 << 62, flag_off=1 << 62)), OK,
        in_bytes=(1 << 62) + span + 40, n_energy=(1 << 62) + span + 1, **far)
    # offsets near 2^62 and 2^63
    add("byte_off 2^62 inside", views_of(view(byte_off=1 << 62)), OK, in_bytes=(1 << 62) + 40, **far, n_energy=16)
    add("byte_off 2^62: one byte short", views_of(view(byte_off=1 << 62)), ELENGTH, in_bytes=(1 << 62) + 39, **far, n_energy=16)
    farther = dict(far, energy_base=(1 << 63) + (1 << 62))
    add("byte_off 2^63 - 1 inside", views_of(view(byte_off=2**63 - 1)), OK, in_bytes=2**63 + 39, **farther, n_energy=16)
    add("byte_off 2^63 - 1: one byte short", views_of(view(byte_off=2**63 - 1)), ELENGTH, in_bytes=2**63 + 38, **farther, n_energy=16)
    add("byte_off 2^63 - 1 with frames beyond 2^63", views_of(view(n_frames=1000, byte_off=2**63 - 1, byte_pitch=M31)), OK,
        in_bytes=2**63 + 999 * M31 + 39, **farther, n_energy=1000)
    add("flag_off 2^63 - 1 inside an energy array of 2^63 floats", views_of(view(flag_off=2**63 - 1)), OK, n_energy=2**63, **far, in_bytes=40)
    add("flag_off 2^63 - 1: one short", views_of(view(flag_off=2**63 - 1)), ELENGTH, n_energy=2**63 - 1, **far, in_bytes=40)
    add("flag_off 2^62 in a spectrum array of 2^62 + 1 rows", views_of(view(flag_off=1 << 62)), OK, in_base=4096, in_bytes=40, flags_base=0, n_flags=0,
        energy_base=0, n_energy=0, bands_base=0, n_bands=0, spec_base=1 << 20, n_spec=(1 << 62) + 1)  # (n_spec * 1600 passes 2^64: taken to the end)
    add("flag_off 2^62 in a band array of 2^62 + 1 rows", views_of(view(flag_off=1 << 62)), OK, in_base=4096, in_bytes=40, flags_base=0, n_flags=0,
        energy_base=0, n_energy=0, spec_base=0, n_spec=0, bands_base=1 << 20, n_bands=(1 << 62) + 1)
    add("an array that ends at 2^64 - 1", views_of(view(byte_off=2**63 - 1, n_frames=M31, byte_pitch=M31)), OK, in_base=1 << 40,
        in_bytes=2**64 - 1 - (1 << 40), flags_base=0, n_flags=0, energy_base=4096, n_energy=M31, **ONLY_ENERGY)
    # address overlaps: each output against d_in, d_bad_frame and the other outputs; touching is no overlap
    E, NE = BOUNDS["energy_base"], BOUNDS["n_energy"]
    add("energy begins inside d_in", views_of(one), EINVAL, in_base=E - 100, in_bytes=101)
    add("energy ends where d_in begins", views_of(one), OK, in_base=E + 4 * NE, in_bytes=4096)
    add("d_in begins inside energy's last float", views_of(one), EINVAL, in_base=E + 4 * NE - 1, in_bytes=4096)
    add("d_in ends where energy begins", views_of(one), OK, in_base=E - 4096, in_bytes=4096)
    add("d_in inside energy", views_of(one), EINVAL, in_base=E + 100, in_bytes=1000)
    add("energy's last byte is the first flag", views_of(one), EINVAL, flags_base=E + 4 * NE - 1)
    add("energy is the flag array", views_of(one), EINVAL, flags_base=E, n_flags=NE)
    add("energy inside the band rows", views_of(one), EINVAL, bands_base=E - 256)
    add("the band rows end where energy begins", views_of(one), OK, bands_base=E - 256 * 64, n_bands=64)
    add("the band rows' last float is energy's first", views_of(one), EINVAL, bands_base=E - 256 * 64 + 4, n_bands=64)
    add("energy inside the spectrum rows", views_of(one), EINVAL, spec_base=E - 1600)
    add("the spectrum rows end where energy begins", views_of(one), OK, spec_base=E - 1600 * 64, n_spec=64)
    add("the band rows inside the spectrum rows", views_of(one), EINVAL, spec_base=BOUNDS["bands_base"] - 1600)
    add("the spectrum rows end where the band rows begin", views_of(one), OK, spec_base=BOUNDS["bands_base"] - 1600 * 64, n_spec=64)
    add("the band rows over d_in", views_of(one), EINVAL, bands_base=BOUNDS["in_base"] + 4096)
    add("the spectrum rows over d_in", views_of(one), EINVAL, spec_base=BOUNDS["in_base"] + 4096)
    add("the band rows over the flags", views_of(one), EINVAL, bands_base=BOUNDS["flags_base"] - 256)
    add("the spectrum rows over the flags", views_of(one), EINVAL, spec_base=BOUNDS["flags_base"] - 1600)
    add("the rows given, the flags not: no flag range to overlap", views_of(one), OK, spec_base=BOUNDS["flags_base"] - 1600, flags_base=0)
    add("an output range of no elements overlaps nothing", views_of(), OK, spec_base=BOUNDS["in_base"], n_spec=0)
    return C


def test_every_refusal_and_every_extreme_has_its_code(emu):
    d = descs_array(DESCS)
    out = np.zeros(2, np.int32)
    seen = set()
    for name, vs, n, b, max_views, max_frames, want in cases():
        rc = emu.lc3emu_av_check(P(d), len(DESCS), max_views, max_frames, P(vs), n, P(b), P(out))
        assert rc == want, (name, rc, want)
        seen.add(want)
        if rc == OK and vs is not None and len(vs):
            assert out[0] == int(vs["n_frames"].astype(np.int64).sum()), name
            assert out[1] == max(int(x["nbytes"]) or 40 for x in vs), name
    assert seen == {OK, EINVAL, ECHANNEL, ELENGTH}


def test_create_refuses_what_the_inspector_refuses_and_max_frames_below_one(emu):
    out = np.zeros(2, np.int32)
    v, b = views_of(view()), bounds()
    for desc, want in (((48000, 10000, 40), OK), ((8000, 7500, 1), OK), ((44100, 10000, 400), OK), ((48000, 5000, 40), EINVAL),
                       ((22050, 10000, 40), EINVAL), ((48000, 10000, 0), ELENGTH), ((48000, 10000, 401), ELENGTH)):
        d = descs_array([desc])
        assert emu.lc3emu_av_check(P(d), 1, 8, 8, P(v), 1, P(b), P(out)) == want, desc
    d = descs_array([(48000, 10000, 40)])
    for mv, mf, want in ((8, 0, EINVAL), (8, -1, EINVAL), (0, 8, EINVAL), (1, 1, OK)):
        assert emu.lc3emu_av_check(P(d), 1, mv, mf, P(v), 1, P(b), P(out)) == want, (mv, mf)


def test_frames_per_workgroup_follow_the_lds_rule(emu):
    """256 lanes, halved down to 64 while 10672 + fpb * (72 + nbytes) + 8 bytes pass 64 KB"""
    for nb in range(1, 401):
        fpb = 256
        while fpb > 64 and 10672 + fpb * (72 + nb) + 8 > 65536:
            fpb //= 2
        assert emu.lc3emu_av_fpb(nb) == fpb, nb
        assert emu.lc3emu_av_lds(nb) == 10672 + fpb * (72 + nb) + 8 <= 65536, nb
    assert [emu.lc3emu_av_fpb(nb) for nb in (1, 142, 143, 356, 357, 400)] == [256, 256, 128, 128, 64, 64]


def _run(emu, descs, vs, d_in, flags, n_out, want=("e", "b", "s"), max_frames=None, in_bytes=None):
    d = descs_array(descs)
    e = np.full(n_out, A.SENTINEL, np.float32)
    b = np.full((n_out, A.BANDS), A.SENTINEL, np.float32)
    s = np.full((n_out, A.LINES), A.SENTINEL, np.float32)
    total = int(vs["n_frames"].astype(np.int64).sum())
    rc = emu.lc3emu_av_run(P(d), len(descs), len(vs), total if max_frames is None else max_frames, P(vs), len(vs), P(d_in),
                           d_in.size if in_bytes is None else in_bytes, P(flags), 0 if flags is None else n_out,
                           P(e) if "e" in want else None, n_out, P(b) if "b" in want else None, n_out, P(s) if "s" in want else None, n_out)
    return rc, e, b, s


def test_the_lane_body_through_the_plan_over_the_corpus_of_all_twelve_configurations(emu):
    """every frame of the corpus, none left out: one call per configuration, a view per frame (so that every size meets the plan), the whole
    output arrays compared"""
    seen = dict(tns2=0, lsb=0, zero=0, nres=0)
    for ch, (fs, us) in enumerate(I.CONFIGS):
        frames, exp = A.config_frames(fs, us), A.config_expected(fs, us)
        good = sum(1 for x in exp if x[0] == 0)
        assert good >= 20 and len(exp) - good >= 5, (fs, us, good, len(exp))
        for st, info, _, _, _ in exp:
            if st == 0:
                seen["tns2"] += info["tns"] == 2
                seen["lsb"] += info["lsb_mode"] == 1
                seen["zero"] += info["zero"] == 1
                seen["nres"] += info["nres"] > 0
        n = len(frames)
        rng = np.random.default_rng(ch)
        order = rng.permutation(n)  # (the frames lie in another order than their outputs)
        offs = np.zeros(n, np.int64)
        pos = 5
        for k in order:
            offs[k] = pos
            pos += len(frames[k][0]) + int(rng.integers(0, 9))
        d_in = np.full(pos + 3, 0xEE, np.uint8)
        flags = np.ones(2 * n + 4, np.uint8)
        vs = []
        for k, (fr, fl) in enumerate(frames):
            d_in[offs[k]: offs[k] + len(fr)] = np.frombuffer(fr, np.uint8)
            flags[2 * k + 1] = fl
            vs.append(view(channel=0, n_frames=1, nbytes=len(fr), byte_off=int(offs[k]), flag_off=2 * k + 1))
        vs = views_of(*vs)
        n_out = 2 * n + 4
        rc, e, b, s = _run(emu, [(fs, us, 40)], vs, d_in, flags, n_out)
        assert rc == OK
        we = np.full(n_out, A.SENTINEL, np.float32)
        wb = np.full((n_out, A.BANDS), A.SENTINEL, np.float32)
        ws = np.full((n_out, A.LINES), A.SENTINEL, np.float32)
        for k, (st, _, te, tb, ts) in enumerate(exp):
            we[2 * k + 1], wb[2 * k + 1], ws[2 * k + 1] = te, tb, ts
        bad_rows = np.nonzero((s.view(np.uint32) != ws.view(np.uint32)).any(1))[0]
        assert not len(bad_rows), (fs, us, bad_rows[:4])
        bad_rows = np.nonzero((b.view(np.uint32) != wb.view(np.uint32)).any(1))[0]
        assert not len(bad_rows), (fs, us, bad_rows[:4], b[bad_rows[0]][:8], wb[bad_rows[0]][:8])
        assert A.same_bits(e, we), (fs, us, np.nonzero(e.view(np.uint32) != we.view(np.uint32))[0][:8])
        # d_energy < 0 exactly where the oracle's status is non-zero
        idx = 2 * np.arange(n) + 1
        assert np.array_equal(e[idx] < 0, np.array([x[0] != 0 for x in exp]))
    assert all(v >= 1 for v in seen.values()), seen


def test_output_forms_rings_and_refusals_write_nothing_else(emu):
    """a small tick in rings (a wrapping ring: one channel in two views) over four configurations: each of the seven output combinations
    gives the same values and leaves the others untouched; without flags the flagged frames are analysed; a refused call writes nothing"""
    rng = np.random.default_rng(5)
    cfgs = [(8000, 7500), (16000, 10000), (44100, 7500), (48000, 10000)]
    descs = [(fs, us, 57) for fs, us in cfgs]
    items = []
    for ch, (fs, us) in enumerate(cfgs):
        by = {}
        for fr, fl in A.config_frames(fs, us):
            by.setdefault(len(fr), []).append((fr, fl))
        for size in sorted(by)[:6]:
            items.append((ch, size, by[size][:int(rng.integers(1, 9))]))
    vs, d_in, flags, n_out, placed = A.ring_tick(items, rng=rng)
    assert len(vs) > len(items)  # some ring wrapped
    we, wb, ws = A.expected_outputs(placed, descs, n_out)
    total = int(vs["n_frames"].sum())
    for want in (("e",), ("b",), ("s",), ("e", "b"), ("e", "s"), ("b", "s"), ("e", "b", "s")):
        rc, e, b, s = _run(emu, descs, vs, d_in, flags, n_out, want)
        assert rc == OK
        for name, got, exp in (("e", e, we), ("b", b, wb), ("s", s, ws)):
            assert A.same_bits(got, exp if name in want else np.full_like(exp, A.SENTINEL)), (want, name)
    we2, wb2, ws2 = A.expected_outputs(placed, descs, n_out, use_flags=False)
    rc, e, b, s = _run(emu, descs, vs, d_in, None, n_out)
    assert rc == OK and A.same_bits(e, we2) and A.same_bits(b, wb2) and A.same_bits(s, ws2)
    for kw in (dict(max_frames=total - 1), dict(in_bytes=int(vs["byte_off"].max()))):
        rc, e, b, s = _run(emu, descs, vs, d_in, flags, n_out, **kw)
        assert rc == ELENGTH and (e == A.SENTINEL).all() and (b == A.SENTINEL).all() and (s == A.SENTINEL).all()
    rc, e, b, s = _run(emu, descs, vs, d_in, flags, n_out, max_frames=total)
    assert rc == OK and A.same_bits(e, we)


def test_the_check_and_the_plan_under_address_and_undefined_behaviour_sanitizers():
    """the stand-alone program (its own main, nothing preloaded, nothing loaded into Python) over the same extreme lists, as a child process"""
    src = os.path.join(EMU_DIR, "lc3_analyze_views_check_main.cpp")
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
            vs = views_of(*[view(channel=int(rng.integers(12)), n_frames=int(rng.integers(1, 400)), nbytes=int(rng.choice([0, 1, 7, 142, 143, 357, 400])),
                                 byte_off=int(rng.integers(0, 1000)), flag_off=int(rng.integers(0, 1000)), flag_pitch=int(rng.integers(0, 4)))
                            for _ in range(int(rng.integers(1, 60)))])
            todo.append(("random", vs, len(vs), bounds(in_bytes=1 << 20, n_flags=4096, n_energy=4096, n_bands=4096, n_spec=4096), 64,
                         int(vs["n_frames"].sum()), OK))
        blob = struct.pack("<i", len(todo))
        for name, vs, n, b, max_views, max_frames, want in todo:
            blob += struct.pack("<i", len(DESCS)) + descs_array(DESCS).tobytes() + struct.pack("<iii", max_views, max_frames, n)
            blob += (vs.tobytes() if n > 0 else b"") + b.tobytes() + struct.pack("<i", want)
        with open(case_file, "wb") as f:
            f.write(blob)
        r = subprocess.run([exe, case_file], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        words = r.stdout.split()
        assert words[0] == "ok" and int(words[1]) == len(todo) and int(words[2]) > 10000, r.stdout
