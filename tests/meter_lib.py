"""Shared pieces of the tests of lc3gpu_measure_mixed_views (the emulator tests and the GPU tests): the model of the call -- the formulas of
include/lc3gpu.h in Python integers and numpy int64 --, a builder of PCM rings and views from a seed, and sentinel-ringed outputs.  Test
infrastructure only."""
import importlib

import numpy as np

import mix_lib as M
from mix_lib import view, views_of

api = importlib.import_module("lc3-codec_amd.api")

CONFIGS = M.CONFIGS  # the twelve (fs_hz, frame_us)
nf_of = M.nf_of
ACTIVE_SENTINEL = 0xA5
LEVEL_SENTINEL = 0x5C  # every byte of an untouched record


def desc(fs, us, attack=16384, release=2048, threshold=1 << 16, hang=2):
    return (fs, us, attack, release, threshold, hang)


def descs_codec(descs):
    """what mix_lib's placement helpers take"""
    return [(d[0], d[1], 40) for d in descs]


def frame_record(x, before, env0, hang0, d):
    """one frame: x int64[nf], before = x[-1] -> (the record as a dict of Python integers, the state after it)"""
    fs, us, attack, release, threshold, hang_frames = d
    nf = len(x)
    xs = [int(v) for v in x]
    sum_sq = sum(v * v for v in xs)
    prev = [int(before)] + xs[:-1]
    ms = sum_sq // nf
    dd = ms - env0
    k = attack if dd > 0 else release
    env = env0 + ((dd * k + 16384) >> 15)
    assert 0 <= env <= 1 << 30 and min(env0, ms) <= env <= max(env0, ms)
    if env >= threshold:
        hang, active = hang_frames, 1
    elif hang0 > 0:
        hang, active = hang0 - 1, 1
    else:
        hang, active = 0, 0
    rec = dict(sum_sq=sum_sq, env=env, sum=sum(xs), min=min(xs), max=max(xs), n_clipped=sum(v in (32767, -32768) for v in xs),
               n_cross=sum((a < 0) != (b < 0) for a, b in zip(xs, prev)), hang=hang, active=active, reserved0=0, reserved1=0)
    return rec, (xs[-1], env, hang)


class Model:
    """the meter's channels: descs = [(fs_hz, frame_us, attack_q15, release_q15, threshold, hang_frames), ...], a state per channel"""

    def __init__(self, descs):
        self.descs = [tuple(int(x) for x in d) for d in descs]
        self.codec = descs_codec(self.descs)
        self.state = [(0, 0, 0) for _ in self.descs]  # last, env, hang

    def reset(self, channels=None):
        for ch in range(len(self.descs)) if channels is None else channels:
            self.state[ch] = (0, 0, 0)

    def call(self, views, pcm, active=None, levels=None):
        """what the call leaves in the outputs (copies; None stays None); the listed channels advance"""
        pcm = np.asarray(pcm).astype(np.int64)
        a = None if active is None else np.array(active, np.uint8, copy=True)
        lv = None if levels is None else np.array(levels, api.LEVEL_DTYPE, copy=True)
        for v in views:
            ch = int(v["channel"])
            nf = nf_of(*self.descs[ch][:2])
            x = pcm[M.sample_index(v, self.codec)].reshape(int(v["n_frames"]), nf)
            fp = int(v["flag_pitch"]) or 1
            last, env, hang = self.state[ch]
            for t in range(x.shape[0]):
                rec, (last, env, hang) = frame_record(x[t], last, env, hang, self.descs[ch])
                i = int(v["flag_off"]) + t * fp
                if a is not None:
                    a[i] = rec["active"]
                if lv is not None:
                    for k, val in rec.items():
                        lv[i][k] = val
            self.state[ch] = (last, env, hang)
        return a, lv


class Tick:
    """views over one PCM ring and the two sentinel-filled outputs"""

    def __init__(self, descs, views, pcm, active, levels):
        self.descs, self.views, self.pcm, self.active, self.levels = descs, views, pcm, active, levels

    @property
    def max_views(self):
        return max(1, len(self.views))


def blank_outputs(n, rng):
    """sentinel-filled outputs of n indices and a few more behind them"""
    n += int(rng.integers(1, 5))
    active = np.full(n, ACTIVE_SENTINEL, np.uint8)
    levels = np.frombuffer(bytes([LEVEL_SENTINEL]) * (32 * n), api.LEVEL_DTYPE).copy()
    return active, levels


def make_tick(descs, items, rng, data=None, shuffle=True):
    """items: (channel, n_frames[, stride, gap, flag_pitch]) per view, each channel at most once.  data: channel -> the samples (default:
    a level per channel between silence and full scale, so that gates open and close).  The views are named in a shuffled order and their
    output indices lie one behind the other with gaps."""
    codec = descs_codec(descs)
    ring = M._Ring(rng)
    vs, xs, flag = [], [], int(rng.integers(0, 4))
    for it in items:
        ch, T = it[0], it[1]
        stride, gap, fp = (tuple(it[2:]) + (1, 0, 0))[:3]
        v = ring.place(ch, T, stride, gap, codec)
        v[0]["flag_off"], v[0]["flag_pitch"] = flag, fp
        flag += (T - 1) * (fp or 1) + 1 + int(rng.integers(0, 3))
        S = T * nf_of(*codec[ch][:2])
        if data is None or ch not in data:
            amp = int(rng.choice([0, 30, 900, 32768]))
            x = rng.integers(-amp, amp, S) if amp else np.zeros(S, np.int64)
        else:
            x = np.resize(np.asarray(data[ch], np.int64), S)
        vs.append(v), xs.append(x)
    pcm = rng.integers(-32768, 32768, ring.cursor + 2 * int(rng.integers(1, 9))).astype(np.int16)  # (noise between the views)
    for v, x in zip(vs, xs):
        pcm[M.sample_index(v[0], codec)] = x.astype(np.int16)
    active, levels = blank_outputs(flag, rng)
    order = rng.permutation(len(vs)) if shuffle else np.arange(len(vs))
    return Tick(list(descs), views_of(*[vs[int(k)] for k in order]), pcm, active, levels)
