"""Shared pieces of the tests of lc3gpu_resample_mixed_views (the table tests, the emulator tests and the GPU tests): the numpy model of the
call -- the formulas of include/lc3gpu.h in int64, the coefficients read from the COMMITTED header tables/lc3_resample_tables.h -- and a
builder of rings and pairs of views from a seed.  Test infrastructure only."""
import math
import os
import re

import numpy as np

import mix_lib as M
from mix_lib import view, views_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "tables", "lc3_resample_tables.h")
SENTINEL = M.SENTINEL
RATES5 = (8000, 16000, 24000, 32000, 48000)
RATES6 = (8000, 16000, 24000, 32000, 44100, 48000)
PAIRS = [(fi, fo) for fi in RATES5 for fo in RATES5 if fi != fo]  # the 20 conversions
COPIES = [(f, f) for f in RATES6]
nf_of = M.nf_of
_tables = None


def ratio_of(fs_in, fs_out):
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g  # L, M


def tables():
    """(L, M) -> int64[L][T], parsed from the committed header (read-only)"""
    global _tables
    if _tables is None:
        with open(HEADER) as f:
            text = f.read()
        meta = re.search(r"lc3_rs_ratios\[LC3_RS_RATIOS\] = \{(.*?)\};", text, re.S).group(1)
        rows = [tuple(int(x) for x in m) for m in re.findall(r"\{(\d+), (\d+), (\d+), (\d+)\}", meta)]
        body = re.search(r"lc3_rs_coef\[LC3_RS_COEF_TOTAL\] = \{(.*?)\};", text, re.S).group(1)
        body = re.sub(r"//[^\n]*", "", body)
        coef = np.array([int(x) for x in re.findall(r"-?\d+", body)], np.int64)
        assert len(coef) == int(re.search(r"#define LC3_RS_COEF_TOTAL (\d+)", text).group(1))
        _tables = {}
        for L, Mm, T, off in rows:
            t = coef[off:off + L * T].reshape(L, T).copy()
            t.setflags(write=False)
            _tables[(L, Mm)] = t
    return _tables


def taps_of(fs_in, fs_out):
    return 1 if fs_in == fs_out else tables()[ratio_of(fs_in, fs_out)].shape[1]


def resample(x, hist, fs_in, fs_out):
    """x: the input in time order; hist: the T - 1 samples before it -> (out int16, new history); int64 throughout, floor shift"""
    x = np.asarray(x, np.int64)
    if fs_in == fs_out:
        return x.astype(np.int16), np.zeros(0, np.int64)
    L, Mm = ratio_of(fs_in, fs_out)
    c = tables()[(L, Mm)]
    T = c.shape[1]
    xx = np.concatenate([np.asarray(hist, np.int64), x])
    assert len(hist) == T - 1 and len(x) * L % Mm == 0
    m = np.arange(len(x) * L // Mm, dtype=np.int64)
    u = m * Mm
    p, b = u % L, u // L
    acc = (c[p] * xx[(T - 1) + b[:, None] - np.arange(T)[None, :]]).sum(axis=1)
    assert np.abs(acc).max(initial=0) < 2**31 - 16384  # (what keeps the device's int32 exact)
    return np.clip((acc + 16384) >> 15, -32768, 32767).astype(np.int16), xx[len(xx) - (T - 1):]


class Model:
    """the resampler's channels: descs = [(fs_in, fs_out, frame_us), ...], a history per channel, zeros when fresh"""

    def __init__(self, descs):
        self.descs = [tuple(int(x) for x in d) for d in descs]
        self.descs_in = [(fi, us, 40) for fi, fo, us in self.descs]   # (what mix_lib's placement helpers take)
        self.descs_out = [(fo, us, 40) for fi, fo, us in self.descs]
        self.hist = [np.zeros(taps_of(fi, fo) - 1, np.int64) for fi, fo, us in self.descs]

    def reset(self, channels=None):
        for ch in range(len(self.descs)) if channels is None else channels:
            self.hist[ch][:] = 0

    def call(self, in_views, pcm_in, out_views, pcm_out):
        """what the call leaves in pcm_out (a copy); the listed channels advance"""
        want = np.array(pcm_out, np.int16, copy=True)
        pcm_in = np.asarray(pcm_in)
        for a, b in zip(in_views, out_views):
            ch = int(a["channel"])
            fi, fo, us = self.descs[ch]
            out, self.hist[ch] = resample(pcm_in[M.sample_index(a, self.descs_in)], self.hist[ch], fi, fo)
            want[M.sample_index(b, self.descs_out)] = out
        return want


class Tick:
    """pairs of views over two rings (the output ring sentinel-filled)"""

    def __init__(self, descs, in_views, pcm_in, out_views, pcm_out):
        self.descs, self.in_views, self.pcm_in, self.out_views, self.pcm_out = descs, in_views, pcm_in, out_views, pcm_out

    @property
    def max_views(self):
        return max(1, len(self.in_views))


def make_tick(descs, items, rng, data=None, shuffle=True):
    """items: (channel, n_frames[, in_stride, in_gap, out_stride, out_gap]) per pair, each channel at most once.  data: channel -> the
    input samples (default: uniform over the whole int16 range).  The pairs are named in a shuffled order."""
    mod = Model(descs)
    ring_in, ring_out = M._Ring(rng), M._Ring(rng)
    vin, vout, xs = [], [], []
    for it in items:
        ch, T = it[0], it[1]
        si, gi, so, go = (tuple(it[2:]) + (1, 0, 1, 0))[:4] if len(it) > 2 else (1, 0, 1, 0)
        a = ring_in.place(ch, T, si, gi, mod.descs_in)
        b = ring_out.place(ch, T, so, go, mod.descs_out)
        S = T * nf_of(*mod.descs_in[ch][:2])
        x = rng.integers(-32768, 32768, S) if data is None or ch not in data else np.resize(np.asarray(data[ch], np.int64), S)
        vin.append(a), vout.append(b), xs.append(x)
    pcm_in = rng.integers(-32768, 32768, ring_in.cursor + 2 * int(rng.integers(1, 9))).astype(np.int16)  # (noise between the views)
    for a, x in zip(vin, xs):
        pcm_in[M.sample_index(a[0], mod.descs_in)] = x.astype(np.int16)
    pcm_out = np.full(ring_out.cursor + 2 * int(rng.integers(1, 9)), SENTINEL, np.int16)
    order = rng.permutation(len(vin)) if shuffle else np.arange(len(vin))
    return Tick(list(descs), views_of(*[vin[int(k)] for k in order]), pcm_in, views_of(*[vout[int(k)] for k in order]), pcm_out)


def any_place(rng):
    """(in_stride, in_gap, out_stride, out_gap): planar compact, planar pitched, strided"""
    si, so = int(rng.choice([1, 1, 2, 8])), int(rng.choice([1, 1, 2, 8]))
    return si, int(rng.choice([0, 6, 38])), so, int(rng.choice([0, 6, 38]))
