"""Batch calls over a list of a MIXED handle's streams (lc3gpu_encode_mixed_list / lc3gpu_decode_mixed_list) through the device headers under
the CPU wave emulator: tests/emu/lc3_emu_mixed_list.cpp builds every tick's plan with lc3_host_mixed_list.h -- the header the library's host
side builds it with -- and runs the three stream bodies of lc3_dev_list.h as the mixed-list kernels call them, group by group, over a
persistent array of channel states in the handle's internal order.  The yardstick is one oracle encoder / decoder per channel LIFE at the
channel's own (fs, frame_us, nbytes); a reset channel gets a new oracle object.
The handle holds three groups, one of them 7.5 ms, interleaved in the caller's order.  Ticks list 1, 2, 3, 4 and 5 streams of a group, so
that partial workgroups sit in the middle of the grid (the scenario asserts that every count occurs and the emulator reports the mid-grid
partial workgroups it ran); channels are reset between ticks so that fresh and carried streams share workgroups; the decoder sees flagged
and corrupt frames.  Checked: byte-identical frames and sample-identical PCM per (channel, that channel's k-th frame), the state blobs of
unlisted channels byte for byte, and the spare plane columns' pre-filled pattern.  A per-stream branch around a workgroup barrier
deadlocks the emulator: the run goes in a child process with a time limit."""
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
LIB = os.path.join(EMU_DIR, "liblc3emu_mixed_list.so")
synth = importlib.import_module("lc3-codec_amd.synth")
TIME_LIMIT = 1500
FS_ORDER = [8000, 16000, 24000, 32000, 44100, 48000]
# three groups, interleaved in the caller's order: 48 kHz / 10 ms at 100 bytes, 48 kHz / 7.5 ms at 80 bytes, 16 kHz / 10 ms at 40 bytes
KINDS = [(48000, 10000, 100), (48000, 7500, 80), (16000, 10000, 40)]
PER_KIND = [6, 6, 5]


def _build():
    srcs = [os.path.join(EMU_DIR, "lc3_emu_mixed_list.cpp"), os.path.join(EMU_DIR, "lc3_emu.cpp"), os.path.join(ROOT, "tables", "lc3_tables.h")]
    csrc = os.path.join(ROOT, "lc3-codec_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in srcs):
        return LIB
    tmp = LIB + ".tmp%d" % os.getpid()
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-strict-aliasing",
                           "-Wno-unknown-pragmas", "-Wno-attributes", "-o", tmp, srcs[0], "-lpthread"])
    os.replace(tmp, LIB)
    return LIB


# The child replays the scenario: per tick the list, the channels' fresh flags (the library's host-side record), the ragged PCM, then the
# decoder's flags and the corruption to apply to the encoder's bytes.  It records every tick's bytes and PCM, whether an unlisted
# channel's state blob moved, the spare plane words that changed and the mid-grid partial workgroups it ran.
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
L.lc3emu_ml_encode.argtypes = [vp, vp, i, vp, i, vp, vp, vp]
L.lc3emu_ml_decode.argtypes = [vp, vp, i, vp, i, vp, vp, vp, i, vp]
L.lc3emu_ml_state.argtypes = [vp, i, i, vp]
L.lc3emu_ml_free.argtypes = [vp]
L.lc3emu_ml_group_of.argtypes = [vp, i]
p = lambda a: a.ctypes.data_as(vp)
h = L.lc3emu_ml_new(n_ch, p(descs))
assert h
def states(dec):
    n = L.lc3emu_ml_state_size(dec)
    out = np.zeros((n_ch, n), np.uint8)
    for c in range(n_ch):
        L.lc3emu_ml_state(h, dec, c, p(out[c]))
    return out
res = {"group_of": np.array([L.lc3emu_ml_group_of(h, c) for c in range(n_ch)])}
touched = spare = partials = 0
for k in range(int(z["n_ticks"])):
    ch = np.ascontiguousarray(z["list_%d" % k], np.int32)
    T = int(z["T_%d" % k])
    pcm = np.ascontiguousarray(z["pcm_%d" % k])
    idle = np.setdiff1d(np.arange(n_ch), ch)
    info = np.zeros(4, np.int32)
    before = states(0)
    out = np.full(int(z["nbytes_total_%d" % k]), 0xA5, np.uint8)
    assert L.lc3emu_ml_encode(h, p(ch), ch.size, p(np.ascontiguousarray(z["enc_fresh_%d" % k])), T, p(pcm), p(out), p(info)) == 0
    touched += int((before[idle] != states(0)[idle]).any())
    spare += int(info[0]); partials += int(info[1])
    res["bytes_%d" % k] = out
    data = np.ascontiguousarray(out ^ z["xor_%d" % k])  # the scenario's corruption
    bad = np.ascontiguousarray(z["bad_%d" % k])
    pcm_out = np.full(pcm.size, 12345, np.int16)
    before = states(1)
    assert L.lc3emu_ml_decode(h, p(ch), ch.size, p(np.ascontiguousarray(z["dec_fresh_%d" % k])), T, p(data), p(bad), p(pcm_out), int(z["late_%d" % k]), p(info)) == 0
    touched += int((before[idle] != states(1)[idle]).any())
    spare += int(info[0]); partials += int(info[1])
    res["pcm_%d" % k] = pcm_out
L.lc3emu_ml_free(h)
res["touched"], res["spare"], res["partials"] = np.array([touched]), np.array([spare]), np.array([partials])
np.savez(path, **res)
"""


def _scenario(seed):
    rng = np.random.default_rng(seed)
    # caller order: the kinds take turns
    descs, kind_of = [], []
    left = list(PER_KIND)
    while any(left):
        for k in range(len(KINDS)):
            if left[k]:
                descs.append(KINDS[k])
                kind_of.append(k)
                left[k] -= 1
    n_ch = len(descs)
    members = [[c for c in range(n_ch) if kind_of[c] == k] for k in range(len(KINDS))]
    # listed streams per kind, frames, the synthesis form
    shape = [((5, 5, 5), 2, 0), ((1, 2, 3), 1, 1), ((4, 0, 1), 2, 0), ((2, 3, 0), 1, 1), ((3, 1, 4), 2, 1), ((0, 4, 2), 1, 0), ((5, 5, 5), 1, 1),
             ((2, 5, 3), 1, 0)]
    ticks = []
    for k, (counts, T, late) in enumerate(shape):
        ch = []
        for kind, n in enumerate(counts):
            ch += [int(c) for c in rng.choice(members[kind], n, replace=False)]
        ch = [int(c) for c in rng.permutation(ch)]  # any order: the plan buckets it
        resets = (lambda: [int(c) for c in rng.choice(n_ch, 6, replace=False)]) if k else (lambda: [])
        ticks.append(dict(channels=ch, T=T, late=late, enc_reset=resets(), dec_reset=resets()))
    return descs, kind_of, ticks, rng


def _group_order(descs):
    """the handle's internal order: stable by (configuration slot, frame bytes), as build_mixed sorts"""
    key = lambda c: (2 * FS_ORDER.index(descs[c][0]) + (descs[c][1] == 10000), descs[c][2])
    return sorted(range(len(descs)), key=key), key


def test_mixed_list_ticks_three_groups():
    descs, kind_of, ticks, rng = _scenario(31)
    n_ch = len(descs)
    nf = [O.Encoder(d[0], d[1]).nf for d in descs]
    total = sum(t["T"] for t in ticks) + 1
    material = []
    per_kind_seen = [0] * len(KINDS)
    for c, d in enumerate(descs):  # the first three streams of a kind carry the LTPF material
        i = per_kind_seen[kind_of[c]]
        per_kind_seen[kind_of[c]] += 1
        material.append(synth.make_ltpf_pcm(nf[c], d[0], n_frames=total)[i] if i < 3 else synth.make_pcm(1, total, nf[c], d[0], seed=100 + c)[0])
    cursor = [0] * n_ch
    enc_fresh, dec_fresh = [True] * n_ch, [True] * n_ch  # the library's host-side record
    enc_or = [O.Encoder(d[0], d[1]) for d in descs]
    dec_or = [O.Decoder(d[0], d[1]) for d in descs]
    _, key = _group_order(descs)
    io = {"n_ticks": len(ticks), "descs": np.array(descs, np.int32)}
    want, counts_seen, mixed_wgs = [], set(), 0
    for k, t in enumerate(ticks):
        for c in t["enc_reset"]:
            enc_fresh[c], enc_or[c] = True, O.Encoder(descs[c][0], descs[c][1])
        for c in t["dec_reset"]:
            dec_fresh[c], dec_or[c] = True, O.Decoder(descs[c][0], descs[c][1])
        ch, T = t["channels"], t["T"]
        # the launch order: the list bucketed by group, stable; workgroups of four inside a group
        for gk in sorted(set(key(c) for c in ch)):
            grp = [c for c in ch if key(c) == gk]
            counts_seen.add(len(grp))
            for w in range(0, len(grp), 4):
                fr = [enc_fresh[c] for c in grp[w:w + 4]]
                mixed_wgs += int(any(fr) and not all(fr))
        io["list_%d" % k], io["T_%d" % k], io["late_%d" % k] = np.array(ch, np.int32), T, t["late"]
        io["enc_fresh_%d" % k], io["dec_fresh_%d" % k] = np.array(enc_fresh, np.uint8), np.array(dec_fresh, np.uint8)
        pcm = [material[c][cursor[c]:cursor[c] + T] for c in ch]
        io["pcm_%d" % k] = np.concatenate([x.reshape(-1) for x in pcm])
        bad = (rng.random((len(ch), T)) < 0.12).astype(np.uint8)
        io["bad_%d" % k] = bad
        ref_bytes, ref_pcm, xors = [], [], []
        for i, c in enumerate(ch):
            nbytes = descs[c][2]
            xor = np.zeros((T, nbytes), np.uint8)
            for j in np.flatnonzero(rng.random(T) < 0.15):
                xor[j, rng.integers(0, nbytes, 3)] = rng.integers(1, 256, 3)
            rb, rp = np.zeros((T, nbytes), np.uint8), np.zeros((T, nf[c]), np.int16)
            for j in range(T):
                rb[j] = enc_or[c].encode_frame(pcm[i][j], nbytes)
                buf = rb[j] ^ xor[j]
                if bad[i, j]:
                    buf[-2:] = 0xFF  # (the oracle has no external flag: unparsable side information at the frame's own size)
                _, rp[j] = dec_or[c].decode_frame(buf)
                assert not bad[i, j] or dec_or[c].last_was_plc(), "the oracle must conceal what stands for a flagged frame"
            cursor[c] += T
            enc_fresh[c] = dec_fresh[c] = False
            ref_bytes.append(rb.reshape(-1))
            ref_pcm.append(rp.reshape(-1))
            xors.append(xor.reshape(-1))
        io["xor_%d" % k] = np.concatenate(xors)
        io["nbytes_total_%d" % k] = sum(x.size for x in ref_bytes)
        want.append((ref_bytes, ref_pcm))
    assert {1, 2, 3, 4, 5} <= counts_seen, "the scenario must list 1, 2, 3, 4 and 5 streams of a group: %s" % sorted(counts_seen)
    assert mixed_wgs >= 5, "the scenario must put fresh and carried streams into the same workgroups (%d)" % mixed_wgs
    assert any(d[1] == 7500 for d in descs) and len(set(descs)) >= 3
    lib = _build()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "io.npz")
        np.savez(path, **io)
        try:
            r = subprocess.run([sys.executable, "-c", _CHILD, lib, path], timeout=TIME_LIMIT, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.fail("mixed-list emulator run did not finish in %d s: a per-stream branch around a workgroup barrier?" % TIME_LIMIT)
        assert r.returncode == 0, r.stderr[-2000:]
        z = np.load(path)
        # the emulator's handle sorted the streams into the groups this test assumed
        order, _ = _group_order(descs)
        assert [int(g) for g in z["group_of"]] == [sorted(set(key(c) for c in range(n_ch))).index(key(c)) for c in range(n_ch)]
        for k, (ref_bytes, ref_pcm) in enumerate(want):
            ch = ticks[k]["channels"]
            got_b, got_p = z["bytes_%d" % k], z["pcm_%d" % k]
            assert got_b.size == sum(x.size for x in ref_bytes) and got_p.size == sum(x.size for x in ref_pcm)
            ob = op = 0
            for i, c in enumerate(ch):
                assert np.array_equal(got_b[ob:ob + ref_bytes[i].size], ref_bytes[i]), "tick %d: bytes of list item %d (channel %d) differ from the oracle" % (k, i, c)
                assert np.array_equal(got_p[op:op + ref_pcm[i].size], ref_pcm[i]), "tick %d: PCM of list item %d (channel %d) differs from the oracle" % (k, i, c)
                ob += ref_bytes[i].size
                op += ref_pcm[i].size
        assert int(z["touched"][0]) == 0, "a channel that a tick did not list changed its state blob"
        assert int(z["spare"][0]) == 0, "plane columns outside the listed frames were written"
        assert int(z["partials"][0]) >= 5, "partial workgroups in the middle of the grid"
