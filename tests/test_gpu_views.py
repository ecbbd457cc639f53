"""lc3gpu_encode_mixed_views / lc3gpu_decode_mixed_views on the GPU: every item of a mixed handle's tick with the placement of its PCM, its
frames and its flags, read and written in place.  Yardsticks: one oracle encoder / decoder per channel LIFE, called frame by frame (a
reset channel gets a new oracle object); lc3gpu_*_mixed_items on twin handles for placements that are its prefix sums;
lc3gpu_*_mixed_mc_items on twin handles for placements that spell out its layout.  After every call on rings the WHOLE output buffer is
compared: the frames' own bytes / samples are the yardstick's, every other element still holds its sentinel (0xA5 / 12345)."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_items as IT
import test_gpu_mc_items as MC
import test_gpu_mixed_list as ML

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")
synth = importlib.import_module("lc3-codec_amd.synth")
ROOT, MIXED = ML.ROOT, ML.MIXED
EINVAL, ECHANNEL, ELENGTH = -1, -2, -3
torch_mod, dev, cur_stream, _cat = ML.torch_mod, ML.dev, ML.cur_stream, ML._cat
SLOTS, SLOT_BYTES, HEADER, SLOT_PCM = 8, 400, 12, 480  # a stream's rings: 8 slots of 400 bytes behind a 12-byte header, 8 of 480 samples, 8 flags
BYTE_PITCH = HEADER + SLOT_BYTES


def view(channel, n_frames, pcm_off, byte_off, nbytes=0, pcm_stride=1, flag_off=0, pcm_pitch=0, byte_pitch=0, flag_pitch=0):
    return dict(channel=int(channel), n_frames=int(n_frames), nbytes=int(nbytes), pcm_stride=int(pcm_stride), pcm_off=int(pcm_off),
                byte_off=int(byte_off), flag_off=int(flag_off), pcm_pitch=int(pcm_pitch), byte_pitch=int(byte_pitch), flag_pitch=int(flag_pitch))


class RingServer(IT.ItemsServer):
    """ItemsServer whose data lies in per-stream rings: channel c owns byte slots [c * 8, c * 8 + 8) of 412 bytes (the frame behind a 12-byte
    header), PCM slots of 480 samples whatever nf, and 8 flags.  Items are (channel, n_frames, nbytes) with the DECODER's channel index; a
    tick's frames of a channel start at a random slot that leaves room for them (a tick does not wrap)."""

    def ring_views(self, items, enc):
        out, slots = [], []
        for c, T, nb in items:
            s0 = int(self.rng.integers(0, SLOTS - T + 1))
            slots.append(s0)
            out.append(view(self.enc_index[c] if enc else c, T, (c * SLOTS + s0) * SLOT_PCM, (c * SLOTS + s0) * BYTE_PITCH + HEADER, nbytes=nb,
                            flag_off=c * SLOTS + s0, pcm_pitch=SLOT_PCM, byte_pitch=BYTE_PITCH, flag_pitch=1))
        return out, slots

    def encode(self, items, what=""):
        torch = torch_mod()
        items = [(int(c), int(T), int(nb)) for c, T, nb in items if self.encodable[c]]
        views, slots = self.ring_views(items, True)
        pcm = np.full(self.n_ch * SLOTS * SLOT_PCM, 12345, np.int16)
        want = np.full(self.n_ch * SLOTS * BYTE_PITCH, 0xA5, np.uint8)
        for (c, T, nb), s0 in zip(items, slots):
            for j in range(T):
                x = self.material[c][self.cursor[c] + j]
                at = (c * SLOTS + s0 + j) * SLOT_PCM
                pcm[at:at + self.nf[c]] = x
                fr = self.enc_or[c].encode_frame(x, self.size(c, nb))
                b = (c * SLOTS + s0 + j) * BYTE_PITCH + HEADER
                want[b:b + fr.size] = fr
                self.queue[c].append(np.array(fr, np.uint8))
            self.cursor[c] += T
        d_out = torch.full((want.size,), 0xA5, dtype=torch.uint8, device="cuda")
        self.enc.encode_mixed_views(views, dev(pcm), d_out, stream=cur_stream())
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        for (c, T, nb), s0 in zip(items, slots):
            b = (c * SLOTS + s0) * BYTE_PITCH
            assert np.array_equal(got[b:b + T * BYTE_PITCH], want[b:b + T * BYTE_PITCH]), "%s encode: channel %d %s, %d frames at %d bytes from slot %d differ from the oracle" % (
                what, c, self.descs[c], T, self.size(c, nb), s0)
        assert np.array_equal(got, want), "%s encode: a byte outside the written frames lost its 0xA5" % what

    def decode(self, items, what="", raw=()):
        torch = torch_mod()
        rng = self.rng
        items = [(int(c), int(T), int(nb)) for c, T, nb in items]
        views, slots = self.ring_views(items, False)
        data = rng.integers(0, 256, self.n_ch * SLOTS * BYTE_PITCH).astype(np.uint8)  # headers and idle slots hold anything
        flags = np.ones(self.n_ch * SLOTS, np.uint8)  # ... and idle slots' flags are set
        want = np.full(self.n_ch * SLOTS * SLOT_PCM, 12345, np.int16)
        for (c, T, nb), s0 in zip(items, slots):
            n = self.size(c, nb)
            for j in range(T):
                fr = self.queue[c].pop(0).copy()
                assert fr.size == n
                if rng.random() < 0.12:
                    fr[rng.integers(0, n, 3)] ^= rng.integers(1, 256, 3).astype(np.uint8)
                fl = int(rng.random() < 0.1)
                b = (c * SLOTS + s0 + j) * BYTE_PITCH + HEADER
                data[b:b + n] = fr
                flags[c * SLOTS + s0 + j] = fl
                if fl:
                    fr[-2:] = 0xFF  # (the oracle has no external flag: unparsable side information at the frame's own size)
                _, y = self.dec_or[c].decode_frame(fr)
                assert not fl or self.dec_or[c].last_was_plc()
                self.plc[c] += int(self.dec_or[c].last_was_plc())
                at = (c * SLOTS + s0 + j) * SLOT_PCM
                want[at:at + self.nf[c]] = y
        d_pcm = torch.full((want.size,), 12345, dtype=torch.int16, device="cuda")
        self.dec.decode_mixed_views(views, dev(data), d_pcm, stream=cur_stream(), d_bad_frame=dev(flags))
        torch.cuda.synchronize()
        got = d_pcm.cpu().numpy()
        for (c, T, nb), s0 in zip(items, slots):
            at = (c * SLOTS + s0) * SLOT_PCM
            assert np.array_equal(got[at:at + T * SLOT_PCM], want[at:at + T * SLOT_PCM]), "%s decode: channel %d %s, %d frames at %d bytes into slot %d differ from the oracle" % (
                what, c, self.descs[c], T, self.size(c, nb), s0)
        assert np.array_equal(got, want), "%s decode: a sample outside the written frames lost its 12345" % what


def test_oracle_30_ms_ticks_in_rings():
    """ten encodable configurations on the encoder, twelve on the decoder, two streams each, every stream in rings of its own; four 30 ms
    ticks of 3 or 4 frames, a random fifth of the streams dropped per tick, resets between ticks, a third of the decoder's views take
    fewer frames than owed, some frames damaged and some flagged"""
    sv = RingServer(2, 4 * 4 + 2, seed=11)
    assert len(set(sv.enc.descs)) == 10 and len(set(sv.dec.descs)) == 12 and sv.n_ch == 24
    rng = np.random.default_rng(30)
    jitter = 0
    for k in range(4):
        if k:
            sv.reset_enc([int(c) for c in rng.choice(sv.n_ch, 3, replace=False)])
            sv.reset_dec([int(c) for c in rng.choice(sv.n_ch, 3, replace=False)])
        due = [int(c) for c in rng.permutation(sv.n_ch) if rng.random() >= 0.2]
        owed = lambda c: 4 if sv.descs[c][1] == 7500 else 3
        sv.encode([(c, owed(c), 0) for c in due], "tick %d" % k)
        dec_items = []
        for c in [int(c) for c in rng.permutation(due)]:
            T = min(owed(c), len(sv.queue[c]))
            if rng.random() < 1 / 3:
                T = min(T, int(rng.integers(1, 4)))
                jitter += 1
            dec_items.append((c, T, 0))
        assert len(set(T for _, T, _ in dec_items)) >= 3
        sv.decode(dec_items, "tick %d" % k)
    assert jitter >= 4
    assert sv.dec.plc_events() == sum(sv.plc) > 0, "PLC count over the channels' current lives"
    assert sv.enc.pair_timeouts() == 0 and sv.dec.pair_timeouts() == 0


def _compact(items, descs, nf):
    """the items call's prefix sums as views: stride 1, all pitches 0"""
    out, po, bo, fo = [], 0, 0, 0
    for c, T, nb in items:
        out.append(view(c, T, po, bo, nbytes=nb, flag_off=fo))
        po, bo, fo = po + T * nf[c], bo + T * (nb or descs[c][2]), fo + T
    return out


def test_compact_views_equal_the_items_call():
    """twin handles, the same buffers: bytes, PCM, state blobs and PLC count"""
    torch = torch_mod()
    sizes = (2, 3)
    descs, pcm = ML._twin_setup(3, sum(sizes) + 2, 7)
    n = len(descs)
    nf = [pkg.Lc3Config(d[0], d[1]).nf for d in descs]
    rng = np.random.default_rng(17)
    enc_vw, enc_it, dec_vw, dec_it = pkg.Lc3Encoder.mixed(descs), pkg.Lc3Encoder.mixed(descs), pkg.Lc3Decoder.mixed(descs), pkg.Lc3Decoder.mixed(descs)
    st = cur_stream()
    cursor = [0] * n
    for k, T0 in enumerate(sizes):
        order = [int(c) for c in rng.permutation(n)][: n - 4 * k]
        items = [(c, T0 - int(rng.random() < 0.4), int(rng.integers(20, 401)) if rng.random() < 0.3 else 0) for c in order]
        views = _compact(items, descs, nf)
        if k:
            for h in (enc_vw, enc_it, dec_vw, dec_it):
                h.reset(order[:3])
        d_pcm = dev(_cat([pcm[c][cursor[c]:cursor[c] + T] for c, T, _ in items], np.int16))
        nbytes = sum(T * (nb or descs[c][2]) for c, T, nb in items)
        out_vw, out_it = (torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
        enc_vw.encode_mixed_views(views, d_pcm, out_vw, stream=st)
        enc_it.encode_mixed_items(items, d_pcm, out_it, stream=st)
        torch.cuda.synchronize()
        assert torch.equal(out_vw, out_it), "encode_mixed_views on compact placements differs from encode_mixed_items (tick %d)" % k
        flags = dev((rng.random(sum(T for _, T, _ in items)) < 0.08).astype(np.uint8))
        pcm_vw, pcm_it = (torch.full((d_pcm.numel(),), 12345, dtype=torch.int16, device="cuda") for _ in range(2))
        dec_vw.decode_mixed_views(views, out_it, pcm_vw, stream=st, d_bad_frame=flags)
        dec_it.decode_mixed_items(items, out_it, pcm_it, stream=st, d_bad_frame=flags)
        torch.cuda.synchronize()
        assert torch.equal(pcm_vw, pcm_it), "decode_mixed_views on compact placements differs from decode_mixed_items (tick %d)" % k
        for c, T, _ in items:
            cursor[c] += T
    assert np.array_equal(enc_vw.state_save(), enc_it.state_save()) and np.array_equal(dec_vw.state_save(), dec_it.state_save())
    assert dec_vw.plc_events() == dec_it.plc_events() > 0


def _spell_out(items, descs, nf):
    """an mc call's items as views: channel c of C at bases P, B, F"""
    out, P, B, F = [], 0, 0, 0
    for first, C, T, nb in items:
        n = nb or descs[first][2]
        for c in range(C):
            out.append(view(first + c, T, P + c, B + c * n, nbytes=nb, pcm_stride=C, flag_off=F + c, pcm_pitch=nf[first] * C, byte_pitch=C * n, flag_pitch=C))
        P, B, F = P + T * nf[first] * C, B + T * C * n, F + T * C
    return out


def test_views_spelling_out_mc_items_equal_the_mc_items_call():
    """stereo items, one C = 3 and one C = 1 item on twin handles, the SAME interleaved buffers, flags in the mc layout"""
    torch = torch_mod()
    descs, groups = MC._layout(MIXED[:10])
    n = len(descs)
    nf = [pkg.Lc3Config(d[0], d[1]).nf for d in descs]
    assert sorted(C for _, C in groups) == [1] + [2] * 9 + [3]
    rng = np.random.default_rng(41)
    pcm = [synth.make_pcm(1, 12, nf[c], d[0], seed=300 + c)[0] for c, d in enumerate(descs)]
    enc_vw, enc_mc, dec_vw, dec_mc = pkg.Lc3Encoder.mixed(descs), pkg.Lc3Encoder.mixed(descs), pkg.Lc3Decoder.mixed(descs), pkg.Lc3Decoder.mixed(descs)
    st = cur_stream()
    cursor = [0] * n
    ticks = [[(first, C, MC._owed(descs[first]), 0) for first, C in groups]]
    stereo = [g for g in groups if g[1] == 2]
    listed = [g for g in groups if g[1] != 2] + [stereo[int(i)] for i in rng.permutation(len(stereo))[:6]]  # the C = 3, the C = 1 and six stereo items
    listed = [listed[int(i)] for i in rng.permutation(len(listed))]
    ticks.append([(first, C, 1 + i % 3, (0, 0, 64, 150)[i % 4]) for i, (first, C) in enumerate(listed)])
    assert {C for _, C, _, _ in ticks[1]} == {1, 2, 3}
    for k, items in enumerate(ticks):
        if k:
            for h in (enc_vw, enc_mc, dec_vw, dec_mc):
                h.reset([listed[0][0], listed[2][0] + listed[2][1] - 1])  # single channels of two listed items
        views = _spell_out(items, descs, nf)
        x = [np.stack([pcm[c][cursor[c]:cursor[c] + T] for c in range(first, first + C)], axis=-1) for first, C, T, _ in items]  # [T][nf][C]
        d_pcm = dev(_cat(x, np.int16))
        total = sum(T * C * (nb or descs[first][2]) for first, C, T, nb in items)
        out_vw, out_mc = (torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
        enc_vw.encode_mixed_views(views, d_pcm, out_vw, stream=st)
        enc_mc.encode_mixed_mc_items(items, d_pcm, out_mc, stream=st)
        torch.cuda.synchronize()
        assert torch.equal(out_vw, out_mc), "tick %d: the views call's bytes differ from the mc-items call's" % k
        flags = dev((rng.random(sum(T * C for _, C, T, _ in items)) < 0.08).astype(np.uint8))
        pcm_vw, pcm_mc = (torch.full((d_pcm.numel(),), 12345, dtype=torch.int16, device="cuda") for _ in range(2))
        dec_vw.decode_mixed_views(views, out_mc, pcm_vw, stream=st, d_bad_frame=flags)
        dec_mc.decode_mixed_mc_items(items, out_mc, pcm_mc, stream=st, d_bad_frame=flags)
        torch.cuda.synchronize()
        assert torch.equal(pcm_vw, pcm_mc), "tick %d: the views call's PCM differs from the mc-items call's" % k
        for first, C, T, _ in items:
            for c in range(first, first + C):
                cursor[c] += T
    assert np.array_equal(enc_vw.state_save(), enc_mc.state_save()) and np.array_equal(dec_vw.state_save(), dec_mc.state_save())
    assert dec_vw.plc_events() == dec_mc.plc_events() > 0
    for h in (enc_vw, enc_mc, dec_vw, dec_mc):
        assert h.pair_timeouts() == 0


def test_three_streams_in_a_wide_capture_buffer():
    """PCM int16[T][nf][8]; three streams take channels 1, 4 and 6 (stride 8), two calls so that the second starts from carried state"""
    torch = torch_mod()
    W, taken = 8, (1, 4, 6)
    descs = [(48000, 10000, 150), (48000, 10000, 100), (48000, 10000, 150)]
    nf = 480
    pcm = [synth.make_pcm(1, 5, nf, 48000, seed=70 + c)[0] for c in range(3)]
    enc, dec = pkg.Lc3Encoder.mixed(descs), pkg.Lc3Decoder.mixed(descs)
    enc_or, dec_or = [O.Encoder(48000, 10000) for _ in descs], [O.Decoder(48000, 10000) for _ in descs]
    st = cur_stream()
    at = 0
    for T in (3, 2):
        wide = np.full((T, nf, W), 12345, np.int16)
        for s, ch in enumerate(taken):
            wide[:, :, ch] = pcm[s][at:at + T]
        byte_off = np.cumsum([0] + [T * d[2] for d in descs])
        views = [view(s, T, ch, byte_off[s], pcm_stride=W, pcm_pitch=nf * W) for s, ch in enumerate(taken)]
        d_out = torch.full((int(byte_off[-1]),), 0xA5, dtype=torch.uint8, device="cuda")
        enc.encode_mixed_views(views, dev(wide), d_out, stream=st)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        ref = [np.stack([enc_or[s].encode_frame(np.ascontiguousarray(pcm[s][at + j]), descs[s][2]) for j in range(T)]) for s in range(3)]
        for s in range(3):
            assert np.array_equal(got[byte_off[s]:byte_off[s + 1]].reshape(T, -1), ref[s]), "stream %d (capture channel %d): bytes differ from the oracle" % (s, taken[s])
        d_wide = torch.full((T * nf * W,), 12345, dtype=torch.int16, device="cuda")
        dec.decode_mixed_views(views, d_out, d_wide, stream=st)
        torch.cuda.synchronize()
        want = np.full((T, nf, W), 12345, np.int16)
        for s, ch in enumerate(taken):
            for j in range(T):
                _, want[j, :, ch] = dec_or[s].decode_frame(ref[s][j])
        assert np.array_equal(d_wide.cpu().numpy().reshape(T, nf, W), want), "the de-interleaved channels differ from the oracle, or another channel was written"
        at += T


def test_every_refusal_launches_nothing_and_advances_nothing():
    torch = torch_mod()
    L = pkg.load_library()
    sv = RingServer(1, 10, seed=51, configs=MC.REFUSAL_CONFIGS)  # ten channels, every one encodable
    sv.tick([(0, 1, 0), (3, 2, 0), (7, 1, 0), (8, 2, 0)], "before")
    sv.reset_enc([3, 8])  # pending resets that the refused calls must not consume
    sv.reset_dec([4, 8])
    n_pcm, n_io, n_fl = sv.n_ch * SLOTS * SLOT_PCM, sv.n_ch * SLOTS * BYTE_PITCH, sv.n_ch * SLOTS
    ok = [view(0, 1, 0, HEADER, pcm_pitch=SLOT_PCM, byte_pitch=BYTE_PITCH, flag_pitch=1),
          view(3, 2, 3 * SLOTS * SLOT_PCM, 3 * SLOTS * BYTE_PITCH + HEADER, flag_off=3 * SLOTS, pcm_pitch=SLOT_PCM, byte_pitch=BYTE_PITCH, flag_pitch=1),
          view(7, 1, 7 * SLOTS * SLOT_PCM + 1, 7 * SLOTS * BYTE_PITCH + HEADER, nbytes=64, pcm_stride=2, flag_off=7 * SLOTS, pcm_pitch=2 * sv.nf[7] + 6)]
    d_pcm = dev(np.zeros(n_pcm, np.int16))
    d_out = torch.full((n_io,), 0xA5, dtype=torch.uint8, device="cuda")
    d_flags = dev(np.zeros(n_fl, np.uint8))
    d_pcm_out = torch.full((n_pcm,), 12345, dtype=torch.int16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(cur_stream())
    blobs = lambda: (sv.enc.state_save(), sv.dec.state_save())
    before = blobs()

    def E(views, n=None, pcm=p(d_pcm), out=p(d_out), pe=n_pcm, ob=n_io, h=None, stream=st):
        v = api._view_list(views) if views is not None else None
        return L.lc3gpu_encode_mixed_views(h or sv.enc._h, api._ptr(v), len(v) if n is None else n, pcm, pe, out, ob, stream)

    def D(views, n=None, pcm=p(d_pcm_out), out=p(d_out), pe=n_pcm, ob=n_io, h=None, stream=st, fl=p(d_flags), nfl=n_fl):
        v = api._view_list(views) if views is not None else None
        return L.lc3gpu_decode_mixed_views(h or sv.dec._h, api._ptr(v), len(v) if n is None else n, out, ob, fl, nfl, pcm, pe, stream)

    def with_(i, **kw):
        out = [dict(v) for v in ok]
        out[i].update(kw)
        return out

    for side, call in enumerate((E, D)):
        for bad in (with_(0, channel=-1), with_(1, channel=10), with_(2, channel=3)):
            assert call(bad) == ECHANNEL
        for bad in (with_(1, n_frames=0), with_(2, n_frames=-2), with_(0, nbytes=401), with_(0, nbytes=-5)):
            assert call(bad) == ELENGTH
        if side == 0:  # 1..19 bytes: the encoder refuses them, the decoder takes them
            assert call(with_(0, nbytes=19)) == ELENGTH
        for bad in (with_(0, pcm_stride=0), with_(2, pcm_stride=9), with_(0, pcm_off=-2), with_(1, byte_off=-1), with_(0, pcm_pitch=sv.nf[0] - 2),
                    with_(2, pcm_pitch=2 * sv.nf[7] - 1), with_(1, byte_pitch=sv.descs[3][2] - 1), with_(2, byte_pitch=63), with_(0, pcm_off=1),
                    with_(1, pcm_pitch=SLOT_PCM + 1)):
            assert call(bad) == EINVAL
        v = api._view_list(ok)
        v["reserved"][1][2] = 7
        assert call(v) == EINVAL
        # the extents: one element short of what the views reach, offsets far outside, the overflow cases -- never launched
        assert call(ok, pe=3 * SLOTS * SLOT_PCM) == ELENGTH and call(ok, ob=3 * SLOTS * BYTE_PITCH) == ELENGTH
        last = 7 * SLOTS * SLOT_PCM + 1 + (sv.nf[7] - 1) * 2
        assert call(ok, pe=last) == ELENGTH
        last = 7 * SLOTS * BYTE_PITCH + HEADER + 63
        assert call(ok, ob=last) == ELENGTH
        for bad in (with_(1, pcm_off=n_pcm), with_(1, byte_off=n_io - 10), with_(0, pcm_off=(1 << 62) - 2), with_(0, byte_off=(1 << 63) - 1),
                    with_(1, n_frames=0x7fffffff, pcm_pitch=0x7ffffffe, byte_pitch=0x7fffffff),
                    with_(1, n_frames=SLOTS * (sv.n_ch - 3) + 1)):  # one slot beyond the last ring
            assert call(bad) == ELENGTH
        assert call([dict(ok[0], n_frames=0x7fffffff), ok[1]], pe=1 << 60, ob=1 << 60, **({"nfl": 1 << 60} if side else {})) == ELENGTH  # > 2^31 - 1 frames
        assert call(None, n=3) == EINVAL and call(ok, pcm=None) == EINVAL and call(ok, out=None) == EINVAL and call(ok, n=-1) == EINVAL
        assert call(ok, n=0) == 0  # no views: nothing launched
        assert call(ok[:2], pcm=ctypes.c_void_p((d_pcm if side == 0 else d_pcm_out).data_ptr() + 2)) == EINVAL  # stride 1 on a base that is not 4-byte aligned
        assert call(ok[2:], pcm=ctypes.c_void_p((d_pcm if side == 0 else d_pcm_out).data_ptr() + 1)) == EINVAL  # stride 2 on an odd base
    # the decoder's flags: a negative offset, a pitch below 1, a flag outside [0, n_flags)
    assert D(with_(1, flag_off=-1)) == EINVAL and D(with_(1, flag_pitch=-1)) == EINVAL
    assert D(ok, nfl=7 * SLOTS) == ELENGTH and D(with_(1, flag_off=n_fl - 1)) == ELENGTH and D(with_(0, flag_off=(1 << 62))) == ELENGTH
    uenc = pkg.Lc3Encoder(8, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    udec = pkg.Lc3Decoder(8, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    assert E(ok, h=uenc._h) == EINVAL and D(ok, h=udec._h) == EINVAL  # uniform handles are refused
    with pytest.raises(pkg.Lc3EncoderError) as ei:
        uenc.encode_mixed_views(ok, d_pcm, d_out)
    assert ei.value.code == EINVAL
    with pytest.raises(pkg.Lc3DecoderError) as ei:
        udec.decode_mixed_views(ok, d_out, d_pcm_out)
    assert ei.value.code == EINVAL
    with pytest.raises(pkg.Lc3EncoderError) as ei:  # the Python layer passes the tensors' sizes as the extents
        sv.enc.encode_mixed_views(ok, d_pcm[:7 * SLOTS * SLOT_PCM], d_out)
    assert ei.value.code == ELENGTH
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()  # a bound handle takes the call on its bound stream only
    torch.cuda.synchronize()
    sv.enc.bind_stream(s1.cuda_stream)
    sv.dec.bind_stream(s1.cuda_stream)
    s2p = ctypes.c_void_p(s2.cuda_stream)
    assert E(ok, stream=s2p) == EINVAL and D(ok, stream=s2p) == EINVAL
    sv.enc.bind_stream(s1.cuda_stream, bind=False)
    sv.dec.bind_stream(s1.cuda_stream, bind=False)
    torch.cuda.synchronize()
    assert bool((d_out == 0xA5).all()) and bool((d_pcm_out == 12345).all()), "a refused call wrote to its output"
    after = blobs()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]), "a refused call changed a state blob"
    # nothing was launched, advanced or reset: the next valid ticks give the oracle's bytes, on channels the refused calls named too
    sv.tick([(0, 1, 0), (3, 2, 0), (7, 1, 64), (8, 3, 0), (4, 2, 0)], "after the refused calls")
    sv.tick([(7, 2, 0), (3, 1, 30), (5, 4, 0)], "after the refused calls")


def _pitched(items, descs, nf, pcm_gap=2, byte_gap=3):
    """views with pcm_pitch = nf + pcm_gap and byte_pitch = nbytes + byte_gap, the views one after the other; also the buffers' sizes"""
    out, po, bo, fo = [], 0, 0, 0
    for c, T, nb in items:
        n = nb or descs[c][2]
        out.append(view(c, T, po, bo, nbytes=nb, flag_off=fo, pcm_pitch=nf[c] + pcm_gap, byte_pitch=n + byte_gap))
        po, bo, fo = po + T * (nf[c] + pcm_gap), bo + T * (n + byte_gap), fo + T
    return out, po, bo


def _gather(buf, views, width):
    """the frames' own elements of a pitched buffer, compact in list order (host side)"""
    key_off, key_pitch = ("pcm_off", "pcm_pitch") if buf.dtype == np.int16 else ("byte_off", "byte_pitch")
    return _cat([buf[v[key_off] + t * v[key_pitch]:v[key_off] + t * v[key_pitch] + w] for v, w in zip(views, width) for t in range(v["n_frames"])], buf.dtype)


def _scatter(buf, views, width, compact):
    key_off, key_pitch = ("pcm_off", "pcm_pitch") if buf.dtype == np.int16 else ("byte_off", "byte_pitch")
    at = 0
    for v, w in zip(views, width):
        for t in range(v["n_frames"]):
            buf[v[key_off] + t * v[key_pitch]:v[key_off] + t * v[key_pitch] + w] = compact[at:at + w]
            at += w
    return buf


def _views_vs_items(encs, decs, descs, pcm, cursor, items, rng, what):
    """one tick: the views call on pitched buffers against the items call on compact ones, on twin handles, gathered on the host; what lies
    between the frames keeps its sentinel"""
    torch = torch_mod()
    st = cur_stream()
    nf = [pkg.Lc3Config(d[0], d[1]).nf for d in descs]
    views, n_pcm, n_io = _pitched(items, descs, nf)
    wp, wb = [nf[c] for c, _, _ in items], [nb or descs[c][2] for c, _, nb in items]
    compact = _cat([pcm[c][cursor[c]:cursor[c] + T] for c, T, _ in items], np.int16)
    spread = _scatter(np.full(n_pcm, 12345, np.int16), views, wp, compact)
    out_vw = torch.full((n_io,), 0xA5, dtype=torch.uint8, device="cuda")
    out_it = torch.full((sum(T * w for (_, T, _), w in zip(items, wb)),), 0xA5, dtype=torch.uint8, device="cuda")
    encs[0].encode_mixed_views(views, dev(spread), out_vw, stream=st)
    encs[1].encode_mixed_items(items, dev(compact), out_it, stream=st)
    torch.cuda.synchronize()
    g_vw, g_it = out_vw.cpu().numpy(), out_it.cpu().numpy()
    assert np.array_equal(_gather(g_vw, views, wb), g_it), "%s: the views call's bytes differ from the items call's" % what
    assert np.array_equal(g_vw, _scatter(np.full(n_io, 0xA5, np.uint8), views, wb, g_it)), "%s: a byte between the frames was written" % what
    fl = (rng.random(sum(T for _, T, _ in items)) < 0.05).astype(np.uint8)
    pcm_vw = torch.full((n_pcm,), 12345, dtype=torch.int16, device="cuda")
    pcm_it = torch.full((compact.size,), 12345, dtype=torch.int16, device="cuda")
    decs[0].decode_mixed_views(views, out_vw, pcm_vw, stream=st, d_bad_frame=dev(fl))
    decs[1].decode_mixed_items(items, out_it, pcm_it, stream=st, d_bad_frame=dev(fl))
    torch.cuda.synchronize()
    g_vw, g_it = pcm_vw.cpu().numpy(), pcm_it.cpu().numpy()
    assert np.array_equal(_gather(g_vw, views, wp), g_it), "%s: the views call's PCM differs from the items call's" % what
    assert np.array_equal(g_vw, _scatter(np.full(n_pcm, 12345, np.int16), views, wp, g_it)), "%s: a sample between the frames was written" % what
    for c, T, _ in items:
        cursor[c] += T


_FORMS_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_views as m
torch = m.torch_mod()
rng = np.random.default_rng(8)
# one tick of two frames per view just above the threshold of the packer / parser forms of full batches, byte_pitch = nbytes + 3 and
# pcm_pitch = nf + 2, against the items call on twin handles
threshold = int(sys.argv[2])
S = threshold // 20 + 1  # ten configurations x S streams x 2 frames > threshold
descs, pcm = m.ML._twin_setup(S, 4, 5, 24)
n = len(descs)
assert 2 * n > threshold and 2 * (n - 10) <= threshold
nf = [m.pkg.Lc3Config(d[0], d[1]).nf for d in descs]
order = [int(c) for c in rng.permutation(n)]
items = [(c, 2, 0) for c in order]
encs = [m.pkg.Lc3Encoder.mixed(descs) for _ in range(2)]
decs = [m.pkg.Lc3Decoder.mixed(descs) for _ in range(2)]
cursor = [0] * n
m._views_vs_items(encs, decs, descs, pcm, cursor, items, rng, "a tick of %d frames" % (2 * n))
assert np.array_equal(encs[0].state_save(), encs[1].state_save()) and np.array_equal(decs[0].state_save(), decs[1].state_save())
assert decs[0].plc_events() == decs[1].plc_events() > 0
# the same tick once more with ONE view at 400 bytes: the launch set's LDS is sized by its largest frame, which takes the pair kernels'
# workgroups beyond 64 KB.  That stream starts a new life and is held to fresh oracle objects, frame by frame
c400 = order[len(order) // 2]
fs, us = descs[c400][0], descs[c400][1]
for h in (encs[0], decs[0]):
    h.reset([c400])
items = [(c, 2, 400 if c == c400 else 0) for c in order]
views, n_pcm, n_io = m._pitched(items, descs, nf)
v = views[order.index(c400)]
x = [pcm[c][cursor[c]:cursor[c] + 2] for c in order]
spread = m._scatter(np.full(n_pcm, 12345, np.int16), views, [nf[c] for c in order], m._cat(x, np.int16))
st = m.cur_stream()
out = torch.full((n_io,), 0xA5, dtype=torch.uint8, device="cuda")
encs[0].encode_mixed_views(views, m.dev(spread), out, stream=st)
torch.cuda.synchronize()
eo = m.O.Encoder(fs, us)
ref = np.stack([eo.encode_frame(np.ascontiguousarray(x[order.index(c400)][j]), 400) for j in range(2)])
got = out.cpu().numpy()
assert np.array_equal(np.stack([got[v["byte_off"] + j * 403:v["byte_off"] + j * 403 + 400] for j in range(2)]), ref), "the 400-byte view's bytes differ from the oracle"
assert (got[v["byte_off"] + 400:v["byte_off"] + 403] == 0xA5).all()
pcm_out = torch.full((n_pcm,), 12345, dtype=torch.int16, device="cuda")
decs[0].decode_mixed_views(views, out, pcm_out, stream=st)
torch.cuda.synchronize()
do = m.O.Decoder(fs, us)
gp = pcm_out.cpu().numpy()
for j in range(2):
    _, want = do.decode_frame(ref[j])
    at = v["pcm_off"] + j * v["pcm_pitch"]
    assert np.array_equal(gp[at:at + nf[c400]], want), "the 400-byte view's PCM differs from the oracle"
    assert (gp[at + nf[c400]:at + v["pcm_pitch"]] == 12345).all()
for h in encs + decs:
    assert h.pair_timeouts() == 0
print("forms ok")
"""


def test_views_every_kernel_form_in_a_fresh_process():
    """one tick of two frames per view just above the full-batch threshold -- the pair packer and parser -- with gaps between the frames,
    against the items call on twin handles, and that tick again with one view at 400 bytes against the oracle, per kernel form, each child
    under its own time limit; stops at the first child that fails"""
    threshold = ML._pc_threshold()
    for env in ML.FORMS:
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", _FORMS_CHILD, ROOT, str(threshold)], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "forms ok" in r.stdout, (env, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
