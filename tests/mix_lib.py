"""Shared pieces of the tests of lc3gpu_mix_mixed_views (the emulator tests and the GPU tests): the numpy model of the call -- the three
formulas of include/lc3gpu.h in int64 -- and a builder of rings, views and room tables from a seed.  Test infrastructure only."""
import importlib

import numpy as np

api = importlib.import_module("lc3-codec_amd.api")

UNITY = 16384
SENTINEL = 0x5A5B  # what an untouched output sample holds (odd halves: a 32-bit store of one sample too many shows)
CONFIGS = [(fs, us) for fs in (8000, 16000, 24000, 32000, 44100, 48000) for us in (7500, 10000)]
DESCS = [(fs, us, 40) for fs, us in CONFIGS]


def nf_of(fs, us):
    """the frame length (common/config.rs:42-100)"""
    nf10 = 480 if fs == 44100 else fs // 100
    return nf10 if us == 10000 else nf10 * 3 // 4


def channel_of(fs, us):
    return CONFIGS.index((fs, us))


def view(channel=0, n_frames=1, pcm_off=0, pcm_stride=1, pcm_pitch=0, reserved=(0, 0, 0), nbytes=0, byte_off=0, byte_pitch=0, flag_off=0,
         flag_pitch=0):
    v = np.zeros(1, api.VIEW_DTYPE)
    for k, x in dict(channel=channel, n_frames=n_frames, nbytes=nbytes, byte_off=byte_off, flag_off=flag_off, byte_pitch=byte_pitch,
                     flag_pitch=flag_pitch, pcm_stride=pcm_stride, pcm_off=pcm_off, pcm_pitch=pcm_pitch).items():
        v[0][k] = x
    v[0]["reserved"] = reserved
    return v


def views_of(*vs):
    return np.ascontiguousarray(np.concatenate(vs)) if vs else np.zeros(0, api.VIEW_DTYPE)


def table(rows, dtype):
    out = np.zeros(len(rows), dtype)
    for k, r in enumerate(rows):
        out[k] = tuple(int(x) for x in r)
    return out


def mix_ins(*rows):
    """(bus, gain_q14) per input view"""
    return table(rows, api.MIX_IN_DTYPE)


def mix_outs(*rows):
    """(bus, minus) per output view"""
    return table(rows, api.MIX_OUT_DTYPE)


def sample_index(v, descs):
    """the element index of every sample s of a view, 0 <= s < S: pcm_off + (s / nf) * pitch + (s % nf) * pcm_stride"""
    nf = nf_of(*descs[int(v["channel"])][:2])
    pitch = int(v["pcm_pitch"]) or nf * int(v["pcm_stride"])
    s = np.arange(int(v["n_frames"]) * nf, dtype=np.int64)
    return int(v["pcm_off"]) + (s // nf) * pitch + (s % nf) * int(v["pcm_stride"])


def model(descs, in_views, ins, pcm_in, out_views, outs, pcm_out):
    """what the call leaves in pcm_out (a copy): term = (in * gain + 8192) >> 14, total = the sum over the bus's inputs, out =
    clamp(total - term(minus)); int64 throughout, floor shifts"""
    pcm_in = np.asarray(pcm_in).astype(np.int64)
    want = np.array(pcm_out, np.int16, copy=True)
    terms = [(pcm_in[sample_index(v, descs)] * int(t["gain_q14"]) + 8192) >> 14 for v, t in zip(in_views, ins)]
    for v, t in zip(out_views, outs):
        idx = sample_index(v, descs)
        total = np.zeros(len(idx), np.int64)
        for i, x in enumerate(ins):
            if int(x["bus"]) == int(t["bus"]):
                total = total + terms[i]
        if int(t["minus"]) >= 0:
            total = total - terms[int(t["minus"])]
        want[idx] = np.clip(total, -32768, 32767).astype(np.int16)
    return want


class Tick:
    """in_views / ins / pcm_in, out_views / outs / pcm_out (sentinel-filled), descs; `want` = model() of them, computed once"""

    def __init__(self, descs, in_views, ins, pcm_in, out_views, outs, pcm_out):
        self.descs, self.in_views, self.ins, self.pcm_in = descs, in_views, ins, pcm_in
        self.out_views, self.outs, self.pcm_out = out_views, outs, pcm_out
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = model(self.descs, self.in_views, self.ins, self.pcm_in, self.out_views, self.outs, self.pcm_out)
            self._want.setflags(write=False)
        return self._want

    @property
    def max_views(self):
        return max(1, len(self.in_views) + len(self.out_views), int(max([0] + [int(b) + 1 for b in self.ins["bus"]] + [int(b) + 1 for b in self.outs["bus"]])))


class _Ring:
    """lays views out one behind the other with gaps, in an array that is wider than what they use"""

    def __init__(self, rng):
        self.rng, self.cursor = rng, 2 * int(rng.integers(1, 9))

    def place(self, ch, T, stride, gap, descs):
        nf = nf_of(*descs[ch][:2])
        pitch = 0 if gap == 0 else nf * stride + gap
        eff = pitch or nf * stride
        off = self.cursor + (int(self.rng.integers(0, stride)) if stride > 1 else 0)
        self.cursor = off + (T - 1) * eff + (nf - 1) * stride + 1 + int(self.rng.integers(0, 7))
        self.cursor += self.cursor & 1
        return view(channel=ch, n_frames=T, pcm_off=off, pcm_stride=stride, pcm_pitch=pitch)


def make_tick(rooms, rng, descs=DESCS, fill="uniform", buses=None):
    """rooms: a list of dict(ins=[...], outs=[...]).  An input is dict(ch, T=1, stride=1, gap=0, gain=UNITY[, data]) or dict(same=(room,
    input), gain=...): the placement of an earlier input once more (one stream feeding two rooms).  An output is dict(ch, T=1, stride=1,
    gap=0, minus=-1) with minus the position of an input WITHIN THE ROOM.  A stride-1 gap is even.  buses: the bus number of every room
    (default: a permutation, so that bus order is not list order).  The views of all rooms are named in a shuffled order."""
    n = len(rooms)
    buses = list(rng.permutation(n)) if buses is None else list(buses)
    ring_in, ring_out = _Ring(rng), _Ring(rng)
    vin, tin, data, where = [], [], [], {}
    for r, room in enumerate(rooms):
        for k, x in enumerate(room["ins"]):
            if "same" in x:
                v = vin[where[x["same"]]].copy()
                d = None
            else:
                v = ring_in.place(x["ch"], x.get("T", 1), x.get("stride", 1), x.get("gap", 0), descs)
                S = int(v[0]["n_frames"]) * nf_of(*descs[x["ch"]][:2])
                d = x.get("data")
                if d is None:
                    d = rng.integers(-32768, 32768, S) if fill == "uniform" else rng.integers(-3000, 3001, S)
                d = np.resize(np.asarray(d, np.int64), S)
            where[(r, k)] = len(vin)
            vin.append(v)
            tin.append((buses[r], x.get("gain", UNITY)))
            data.append(d)
    vout, tout = [], []
    for r, room in enumerate(rooms):
        for x in room["outs"]:
            vout.append(ring_out.place(x["ch"], x.get("T", 1), x.get("stride", 1), x.get("gap", 0), descs))
            m = x.get("minus", -1)
            tout.append((buses[r], where[(r, m)] if m >= 0 else -1))
    pcm_in = rng.integers(-32768, 32768, ring_in.cursor + 2 * int(rng.integers(1, 9))).astype(np.int16)  # (noise between the views)
    for v, d in zip(vin, data):
        if d is not None:
            pcm_in[sample_index(v[0], descs)] = d.astype(np.int16)
    pcm_out = np.full(ring_out.cursor + 2 * int(rng.integers(1, 9)), SENTINEL, np.int16)
    # the tick names its views in any order: shuffle both lists and renumber the minus indices
    pi = rng.permutation(len(vin)) if vin else np.zeros(0, np.int64)
    new_of = {int(old): new for new, old in enumerate(pi)}
    po = rng.permutation(len(vout)) if vout else np.zeros(0, np.int64)
    in_views = views_of(*[vin[int(k)] for k in pi])
    ins = mix_ins(*[tin[int(k)] for k in pi])
    out_views = views_of(*[vout[int(k)] for k in po])
    outs = mix_outs(*[(tout[int(k)][0], new_of[tout[int(k)][1]] if tout[int(k)][1] >= 0 else -1) for k in po])
    return Tick(descs, in_views, ins, pcm_in, out_views, outs, pcm_out)


def n_minus_one_room(chs, rng=None, T=1, listen=False, stride=None, gap=None, gain=UNITY, outs_ch=None):
    """a room of len(chs) participants: every one sends and hears all the others; listen: one more output that hears everybody.  chs:
    (channel, T) pairs or channels; stride / gap: callables of (rng) for variety, or None for planar compact"""
    pick_s = (lambda: int(stride(rng))) if stride else (lambda: 1)
    pick_g = (lambda s: int(gap(rng, s))) if gap else (lambda s: 0)
    ins, outs = [], []
    for k, c in enumerate(chs):
        ch, t = c if isinstance(c, tuple) else (c, T)
        s = pick_s()
        ins.append(dict(ch=ch, T=t, stride=s, gap=pick_g(s), gain=gain))
        s = pick_s()
        outs.append(dict(ch=ch, T=t, stride=s, gap=pick_g(s), minus=k))
    if listen:
        ch, t = chs[0] if isinstance(chs[0], tuple) else (chs[0], T)
        outs.append(dict(ch=ch, T=t, minus=-1))
    return dict(ins=ins, outs=outs)


def gap_any(rng, stride):
    """no gap, or one (even for a planar view)"""
    g = int(rng.choice([0, 0, 6, 38]))
    return g


def stride_any(rng):
    return int(rng.choice([1, 1, 2, 8]))
