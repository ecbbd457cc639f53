"""lc3gpu_encode_mixed_mc_items / lc3gpu_decode_mixed_mc_items on the GPU: items of 1..8 channels of a mixed handle, PCM in WAV sample order
int16[T][nf][C], frames uint8[T][C][nbytes], flags uint8[T][C].  The yardstick is one oracle encoder / decoder per channel LIFE, called
frame by frame (a reset channel gets a new oracle object): identical bytes at [t][c], identical PCM at [t][n][c]; and
lc3gpu_*_mixed_items on twin handles, on the same buffers where every n_channels is 1 and on numpy-de-interleaved buffers otherwise.

An item's channels share one (fs_hz, frame_us) -- the call refuses anything else -- so the one C = 3 item and the one C = 1 item of the
oracle ticks are four streams of ONE configuration (48 kHz / 10 ms); every other configuration has its two streams as a stereo item."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_mixed_list as ML

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("lc3-codec_amd")
ROOT, MIXED = ML.ROOT, ML.MIXED
EINVAL, ECHANNEL, ELENGTH = -1, -2, -3
torch_mod, dev, cur_stream, _cat = ML.torch_mod, ML.dev, ML.cur_stream, ML._cat
WIDE = (48000, 10000, 150)  # the configuration that has four streams: a C = 3 item and a C = 1 item


def _layout(configs):
    """descriptors with the streams of a configuration side by side, and the item groups (first_channel, n_channels) over them"""
    descs, groups = [], []
    for cfg in configs:
        if cfg == WIDE:
            groups += [(len(descs), 3), (len(descs) + 3, 1)]
            descs += [cfg] * 4
        else:
            groups.append((len(descs), 2))
            descs += [cfg] * 2
    return descs, groups


class McServer(ML.MixedServer):
    """MixedServer over a layout of consecutive descriptors per stream, driven by the mc-items calls.  Items are (first_channel, n_channels,
    n_frames, nbytes) with the DECODER's channel indices; the encodable configurations come first, so the encoder's indices are the same."""

    def __init__(self, total_frames, seed, configs=MIXED):
        descs, self.groups = _layout(configs)
        super().__init__(1, total_frames, seed, descs)
        assert all(self.enc_index[c] == c for c in self.enc_channels)

    def size(self, first, nb):
        return nb or self.descs[first][2]

    def tick(self, items, what=""):
        torch = torch_mod()
        rng, st = self.rng, cur_stream()
        items = [tuple(int(v) for v in it) for it in items]
        chans = lambda it: list(range(it[0], it[0] + it[1]))
        x = {it: np.stack([self.material[c][self.cursor[c]:self.cursor[c] + it[2]] for c in chans(it)], axis=-1) for it in items}  # [T][nf][C]
        ref = {}
        enc_items = [it for it in items if self.encodable[it[0]]]
        for it in enc_items:
            first, C, T, nb = it
            ref[it] = np.stack([np.stack([self.enc_or[c].encode_frame(np.ascontiguousarray(x[it][j, :, ci]), self.size(first, nb)) for ci, c in enumerate(chans(it))])
                                for j in range(T)])  # [T][C][nbytes]
        if enc_items:
            d_out = torch.full((sum(ref[it].size for it in enc_items),), 0xA5, dtype=torch.uint8, device="cuda")
            self.enc.encode_mixed_mc_items(enc_items, dev(_cat([x[it] for it in enc_items], np.int16)), d_out, stream=st)
            torch.cuda.synchronize()
            got, off = d_out.cpu().numpy(), 0
            for i, it in enumerate(enc_items):
                g = got[off:off + ref[it].size].reshape(ref[it].shape)
                for ci, c in enumerate(chans(it)):
                    assert np.array_equal(g[:, ci], ref[it][:, ci]), "%s encode: item %d %s, bytes [t][%d] of channel %d %s differ from the oracle" % (
                        what, i, it, ci, c, self.descs[c])
                off += ref[it].size
        data, want, flags = [], [], []
        for it in items:
            first, C, T, nb = it
            n = self.size(first, nb)
            if not self.encodable[first]:  # no reference encoder at 8 kHz: the oracle's batch encoder's frames at the descriptor's size
                assert nb == 0
                fr = np.stack([self.frames8k[c][self.cursor[c]:self.cursor[c] + T] for c in chans(it)], axis=1)
            else:
                fr = ref[it]
            xor = np.zeros((T, C, n), np.uint8)
            for j, ci in zip(*np.nonzero(rng.random((T, C)) < 0.12)):
                xor[j, ci, rng.integers(0, n, 3)] = rng.integers(1, 256, 3)
            fr = fr ^ xor
            fl = (rng.random((T, C)) < 0.1).astype(np.uint8)
            w = np.zeros((T, self.nf[first], C), np.int16)
            for ci, c in enumerate(chans(it)):
                for j in range(T):
                    buf = fr[j, ci].copy()
                    if fl[j, ci]:
                        buf[-2:] = 0xFF  # (the oracle has no external flag: unparsable side information at the frame's own size)
                    _, w[j, :, ci] = self.dec_or[c].decode_frame(buf)
                    assert not fl[j, ci] or self.dec_or[c].last_was_plc()
                    self.plc[c] += int(self.dec_or[c].last_was_plc())
                self.cursor[c] += T
            data.append(fr)
            want.append(w)
            flags.append(fl)
        d_pcm = torch.full((sum(w.size for w in want),), 12345, dtype=torch.int16, device="cuda")
        self.dec.decode_mixed_mc_items(items, dev(_cat(data, np.uint8)), d_pcm, stream=st, d_bad_frame=dev(_cat(flags, np.uint8)))
        torch.cuda.synchronize()
        got, off = d_pcm.cpu().numpy(), 0
        for i, it in enumerate(items):
            g = got[off:off + want[i].size].reshape(want[i].shape)
            for ci, c in enumerate(chans(it)):
                assert np.array_equal(g[:, :, ci], want[i][:, :, ci]), "%s decode: item %d %s, PCM [t][n][%d] of channel %d %s differs from the oracle" % (
                    what, i, it, ci, c, self.descs[c])
            off += want[i].size


def _owed(d):
    return 4 if d[1] == 7500 else 3  # frames in 30 ms


def test_oracle_30_ms_ticks():
    """ten configurations on the encoder, twelve on the decoder, stereo items plus one C = 3 and one C = 1 item; four 30 ms ticks of 3 or 4
    frames, a random fifth of the items dropped per tick, some items at a size of their own, resets between ticks"""
    sv = McServer(4 * 4 + 1, seed=11)
    assert sorted(C for _, C in sv.groups) == [1] + [2] * 11 + [3] and len(set(sv.enc.descs)) == 10 and len(set(sv.dec.descs)) == 12
    rng = np.random.default_rng(30)
    own = 0
    for k in range(4):
        if k:  # single channels of an item may be reset: the others carry on
            sv.reset_enc([int(c) for c in rng.choice(sv.n_ch, 4, replace=False)])
            sv.reset_dec([int(c) for c in rng.choice(sv.n_ch, 4, replace=False)])
        items = []
        for g in rng.permutation(len(sv.groups)):
            first, C = sv.groups[int(g)]
            if C == 2 and rng.random() < 0.2:  # (the C = 3 and the C = 1 item are in every tick)
                continue
            nb = int(rng.integers(20, 401)) if (sv.encodable[first] and rng.random() < 0.25) else 0
            own += nb != 0
            items.append((first, C, _owed(sv.descs[first]), nb))
        assert {C for _, C, _, _ in items} == {1, 2, 3} and {T for _, _, T, _ in items} == {3, 4}
        sv.tick(items, "tick %d" % k)
    assert own >= 3
    assert sv.dec.plc_events() == sum(sv.plc) > 0, "PLC count over the channels' current lives"
    assert sv.enc.pair_timeouts() == 0 and sv.dec.pair_timeouts() == 0


def test_one_channel_items_equal_the_items_call():
    """twin handles, the same buffers: every n_channels 1 is the items call itself"""
    torch = torch_mod()
    sizes = (2, 3)
    descs, pcm = ML._twin_setup(3, sum(sizes) + 2, 7)
    n = len(descs)
    nf = [pkg.Lc3Config(d[0], d[1]).nf for d in descs]
    rng = np.random.default_rng(17)
    enc_mc, enc_it, dec_mc, dec_it = pkg.Lc3Encoder.mixed(descs), pkg.Lc3Encoder.mixed(descs), pkg.Lc3Decoder.mixed(descs), pkg.Lc3Decoder.mixed(descs)
    st = cur_stream()
    cursor = [0] * n
    for k, T0 in enumerate(sizes):
        order = [int(c) for c in rng.permutation(n)][: n - 4 * k]
        items = [(c, T0 - int(rng.random() < 0.4), int(rng.integers(20, 401)) if rng.random() < 0.3 else 0) for c in order]
        if k:
            for h in (enc_mc, enc_it, dec_mc, dec_it):
                h.reset(order[:3])
        d_pcm = dev(_cat([pcm[c][cursor[c]:cursor[c] + T] for c, T, _ in items], np.int16))
        nbytes = sum(T * (nb or descs[c][2]) for c, T, nb in items)
        out_mc, out_it = (torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
        enc_mc.encode_mixed_mc_items([(c, 1, T, nb) for c, T, nb in items], d_pcm, out_mc, stream=st)
        enc_it.encode_mixed_items(items, d_pcm, out_it, stream=st)
        torch.cuda.synchronize()
        assert torch.equal(out_mc, out_it), "encode_mixed_mc_items with n_channels 1 differs from encode_mixed_items (tick %d)" % k
        flags = dev((rng.random(sum(T for _, T, _ in items)) < 0.08).astype(np.uint8))
        pcm_mc, pcm_it = (torch.full((d_pcm.numel(),), 12345, dtype=torch.int16, device="cuda") for _ in range(2))
        dec_mc.decode_mixed_mc_items([(c, 1, T, nb) for c, T, nb in items], out_it, pcm_mc, stream=st, d_bad_frame=flags)
        dec_it.decode_mixed_items(items, out_it, pcm_it, stream=st, d_bad_frame=flags)
        torch.cuda.synchronize()
        assert torch.equal(pcm_mc, pcm_it), "decode_mixed_mc_items with n_channels 1 differs from decode_mixed_items (tick %d)" % k
        for c, T, _ in items:
            cursor[c] += T
    assert np.array_equal(enc_mc.state_save(), enc_it.state_save()) and np.array_equal(dec_mc.state_save(), dec_it.state_save())
    assert dec_mc.plc_events() == dec_it.plc_events() > 0


def _mc_vs_items(encs, decs, descs, pcm, cursor, items, rng, what):
    """one tick: the mc call on interleaved buffers against the items call on the numpy-de-interleaved ones, on twin handles"""
    torch = torch_mod()
    st = cur_stream()
    nf = lambda c: pkg.Lc3Config(descs[c][0], descs[c][1]).nf
    x = [np.stack([pcm[c][cursor[c]:cursor[c] + T] for c in range(first, first + C)], axis=-1) for first, C, T, _ in items]  # [T][nf][C]
    flat = [(c, T, nb) for first, C, T, nb in items for c in range(first, first + C)]
    planar = [x[i][:, :, ci] for i, (first, C, T, _) in enumerate(items) for ci in range(C)]
    sizes = [(T, C, nb or descs[first][2]) for first, C, T, nb in items]
    total = sum(T * C * n for T, C, n in sizes)
    out_mc, out_it = (torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
    encs[0].encode_mixed_mc_items(items, dev(_cat(x, np.int16)), out_mc, stream=st)
    encs[1].encode_mixed_items(flat, dev(_cat(planar, np.int16)), out_it, stream=st)
    torch.cuda.synchronize()
    g_mc, g_it, off = out_mc.cpu().numpy(), out_it.cpu().numpy(), 0
    mux = []
    for T, C, n in sizes:  # the items call's [C][T][n] of an item, multiplexed to [T][C][n]
        mux.append(g_it[off:off + T * C * n].reshape(C, T, n).transpose(1, 0, 2))
        off += T * C * n
    assert np.array_equal(g_mc, _cat(mux, np.uint8)), "%s: the mc call's bytes differ from the items call's, multiplexed" % what
    fl = [(rng.random((T, C)) < 0.05).astype(np.uint8) for T, C, _ in sizes]
    n_pcm = sum(a.size for a in x)
    pcm_mc, pcm_it = (torch.full((n_pcm,), 12345, dtype=torch.int16, device="cuda") for _ in range(2))
    decs[0].decode_mixed_mc_items(items, out_mc, pcm_mc, stream=st, d_bad_frame=dev(_cat(fl, np.uint8)))
    decs[1].decode_mixed_items(flat, out_it, pcm_it, stream=st, d_bad_frame=dev(_cat([f.T for f in fl], np.uint8)))
    torch.cuda.synchronize()
    g_mc, g_it, off = pcm_mc.cpu().numpy(), pcm_it.cpu().numpy(), 0
    ilv = []
    for (first, C, T, _) in items:  # the items call's [C][T][nf] of an item, interleaved to [T][nf][C]
        k = T * C * nf(first)
        ilv.append(g_it[off:off + k].reshape(C, T, -1).transpose(1, 2, 0))
        off += k
    assert np.array_equal(g_mc, _cat(ilv, np.int16)), "%s: the mc call's PCM differs from the items call's, interleaved" % what
    for c, T, _ in flat:
        cursor[c] += T


def test_mc_call_equals_the_items_call_on_de_interleaved_buffers():
    descs, groups = _layout(MIXED[:10])
    n = len(descs)
    rng = np.random.default_rng(41)
    pcm = [importlib.import_module("lc3-codec_amd.synth").make_pcm(1, 12, pkg.Lc3Config(d[0], d[1]).nf, d[0], seed=300 + c)[0] for c, d in enumerate(descs)]
    encs = [pkg.Lc3Encoder.mixed(descs) for _ in range(2)]
    decs = [pkg.Lc3Decoder.mixed(descs) for _ in range(2)]
    cursor = [0] * n
    everyone = [(first, C, _owed(descs[first]), 0) for first, C in groups]
    _mc_vs_items(encs, decs, descs, pcm, cursor, everyone, rng, "all fresh")
    listed = [groups[int(g)] for g in rng.permutation(len(groups))[:7]]
    rest = [c for c in range(n) if not any(first <= c < first + C for first, C in listed)]
    before = [h.state_save(rest) for h in encs + decs]
    for h in encs + decs:
        h.reset([listed[0][0], listed[2][0] + listed[2][1] - 1])  # single channels of two listed items
    items = [(first, C, 1 + i % 3, (0, 0, 64, 150)[i % 4]) for i, (first, C) in enumerate(listed)]
    _mc_vs_items(encs, decs, descs, pcm, cursor, items, rng, "a subset, carried and reset channels")
    for h, b in zip(encs + decs, before):
        assert np.array_equal(h.state_save(rest), b), "channels that were not listed changed"
    assert np.array_equal(encs[0].state_save(), encs[1].state_save()), "encoder blobs of all channels"
    assert np.array_equal(decs[0].state_save(), decs[1].state_save()), "decoder blobs of all channels"
    assert decs[0].plc_events() == decs[1].plc_events()
    for h in encs + decs:
        assert h.pair_timeouts() == 0


REFUSAL_CONFIGS = [(48000, 10000, 150), (48000, 10000, 150), (48000, 10000, 100), (32000, 10000, 80), (32000, 10000, 80), (48000, 7500, 113),
                   (48000, 7500, 113), (16000, 10000, 40), (16000, 10000, 40), (16000, 10000, 40)]


class _FlatServer(McServer):
    def __init__(self, total_frames, seed):
        self.groups = []
        ML.MixedServer.__init__(self, 1, total_frames, seed, REFUSAL_CONFIGS)


def test_every_refusal_launches_nothing_and_advances_nothing():
    torch = torch_mod()
    L = pkg.load_library()
    sv = _FlatServer(10, seed=51)  # ten channels, every one encodable; channels 1 and 2 share a configuration and differ in nbytes
    sv.tick([(0, 2, 1, 0), (3, 2, 2, 0), (7, 3, 1, 0)], "before")
    sv.reset_enc([3, 8])  # pending resets that the refused calls must not consume
    sv.reset_dec([4, 8])
    ok = [(0, 2, 1, 0), (3, 2, 2, 0), (7, 3, 1, 64)]
    arr = lambda it: np.array(it, np.int32)
    nf = sv.nf
    d_pcm = dev(np.zeros(sum(C * T * nf[f] for f, C, T, _ in ok), np.int16))
    d_out = torch.full((sum(C * T * sv.size(f, nb) for f, C, T, nb in ok),), 0xA5, dtype=torch.uint8, device="cuda")
    d_pcm_out = torch.full((d_pcm.numel(),), 12345, dtype=torch.int16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    cp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    st = ctypes.c_void_p(cur_stream())
    E = lambda it, n, a, b, h=None: L.lc3gpu_encode_mixed_mc_items(h or sv.enc._h, it, n, a, b, st)
    D = lambda it, n, a, b, h=None: L.lc3gpu_decode_mixed_mc_items(h or sv.dec._h, it, n, a, None, b, st)
    blobs = lambda: (sv.enc.state_save(), sv.dec.state_save())
    before = blobs()

    def with_(i, **kw):
        a = arr(ok)
        for name, v in kw.items():
            a[i, ("first", "C", "T", "nb").index(name)] = v
        return a

    for side, (call, a, b) in enumerate(((E, p(d_pcm), p(d_out)), (D, p(d_out), p(d_pcm_out)))):
        # a channel range outside [0, n_streams); a channel named by two items
        for bad in (with_(2, first=8), with_(0, first=-1), with_(1, first=10), with_(1, first=1), with_(2, first=4, C=2)):
            assert call(cp(bad), 3, a, b) == ECHANNEL
        for bad in (with_(0, C=0), with_(2, C=9), with_(1, C=-1)):  # n_channels outside 1..8
            assert call(cp(bad), 3, a, b) == EINVAL
        assert call(cp(arr([(2, 2, 1, 90), (7, 3, 1, 64)])), 2, a, b) == EINVAL  # 48 kHz and 32 kHz in one item
        assert call(cp(arr([(4, 2, 1, 90), (7, 3, 1, 64)])), 2, a, b) == EINVAL  # 10 ms and 7.5 ms in one item
        assert call(cp(arr([(1, 2, 1, 0), (7, 3, 1, 64)])), 2, a, b) == ELENGTH  # nbytes 0 while the descriptors' sizes differ
        for bad in (with_(1, T=0), with_(2, T=-2), with_(0, nb=401), with_(0, nb=-5)):
            assert call(cp(bad), 3, a, b) == ELENGTH
        if side == 0:  # 1..19 bytes: the encoder refuses them, the decoder takes them
            assert call(cp(with_(0, nb=19)), 3, a, b) == ELENGTH
        assert call(cp(with_(2, T=0x7fffffff)), 3, a, b) == ELENGTH  # more than 2^31 - 1 channel-frames
        assert call(cp(arr([(0, 2, 0x3fffffff, 0), (3, 2, 1, 0)])), 2, a, b) == ELENGTH
        assert call(None, 3, a, b) == EINVAL
        assert call(cp(arr(ok)), 3, None, b) == EINVAL
        assert call(cp(arr(ok)), 3, a, None) == EINVAL
        assert call(cp(arr(ok)), -1, a, b) == EINVAL
        assert call(cp(arr(ok)), 0, a, b) == 0  # no items: nothing launched
    assert E(cp(arr(ok)), 3, ctypes.c_void_p(d_pcm.data_ptr() + 2), p(d_out)) == EINVAL  # misaligned PCM
    assert D(cp(arr(ok)), 3, p(d_out), ctypes.c_void_p(d_pcm_out.data_ptr() + 2)) == EINVAL
    uenc = pkg.Lc3Encoder(8, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    udec = pkg.Lc3Decoder(8, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    assert E(cp(arr(ok)), 3, p(d_pcm), p(d_out), h=uenc._h) == EINVAL  # uniform handles are refused
    assert D(cp(arr(ok)), 3, p(d_out), p(d_pcm_out), h=udec._h) == EINVAL
    with pytest.raises(pkg.Lc3EncoderError) as ei:
        uenc.encode_mixed_mc_items([(0, 2, 1)], d_pcm, d_out)
    assert ei.value.code == EINVAL
    with pytest.raises(pkg.Lc3DecoderError) as ei:
        udec.decode_mixed_mc_items([(0, 2, 1)], d_out, d_pcm_out)
    assert ei.value.code == EINVAL
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()  # a bound handle takes the call on its bound stream only
    torch.cuda.synchronize()
    sv.enc.bind_stream(s1.cuda_stream)
    sv.dec.bind_stream(s1.cuda_stream)
    s2p = ctypes.c_void_p(s2.cuda_stream)
    assert L.lc3gpu_encode_mixed_mc_items(sv.enc._h, cp(arr(ok)), 3, p(d_pcm), p(d_out), s2p) == EINVAL
    assert L.lc3gpu_decode_mixed_mc_items(sv.dec._h, cp(arr(ok)), 3, p(d_out), None, p(d_pcm_out), s2p) == EINVAL
    sv.enc.bind_stream(s1.cuda_stream, bind=False)
    sv.dec.bind_stream(s1.cuda_stream, bind=False)
    torch.cuda.synchronize()
    assert bool((d_out == 0xA5).all()) and bool((d_pcm_out == 12345).all()), "a refused call wrote to its output"
    after = blobs()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]), "a refused call changed a state blob"
    # nothing was launched, advanced or reset: the next valid calls give the oracle's bytes, on channels the refused calls named too
    sv.tick(ok + [(5, 2, 3, 0)], "after the refused calls")
    # ... and an item whose descriptors differ in nbytes is accepted once it names a size of its own (channels 1 and 2: 150 and 100 bytes)
    sv.tick([(7, 3, 2, 0), (0, 1, 1, 0), (1, 2, 2, 90), (3, 2, 1, 0), (5, 2, 1, 30)], "after the refused calls")


_FORMS_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_mc_items as m
torch = m.torch_mod()
sv = m.McServer(14, seed=3)
rng = np.random.default_rng(8)
for k in range(3):
    if k:
        sv.reset_enc([int(c) for c in rng.choice(sv.n_ch, 3, replace=False)])
        sv.reset_dec([int(c) for c in rng.choice(sv.n_ch, 3, replace=False)])
    chosen = [sv.groups[int(g)] for g in rng.choice(len(sv.groups), int(rng.integers(2, len(sv.groups) + 1)), replace=False)]
    sv.tick([(f, C, int(rng.integers(1, 5)), 0 if (rng.random() < 0.6 or not sv.encodable[f]) else int(rng.integers(20, 401))) for f, C in chosen], "tick %d" % k)
assert sv.dec.plc_events() == sum(sv.plc)
# one stereo tick of two frames per item just above the threshold of the packer / parser forms of full batches, against the items call on
# twin handles: frame (s, 1) of every channel goes through the pair packer and the pair parser at C = 2
threshold = int(sys.argv[2])
S = threshold // 40 + 1  # ten configurations x S streams x 2 channels x 2 frames > threshold channel-frames
descs, pcm = m.ML._twin_setup(S, 4, 5, 24)
descs = [d for d in descs for _ in range(2)]
pcm = [x for x in pcm for _ in range(2)]
n = len(descs)
assert 2 * n > threshold and 2 * (n - 20) <= threshold
pcm[1::2] = [np.roll(x, 7, axis=-1) for x in pcm[1::2]]  # (left and right differ)
order = [int(g) for g in rng.permutation(n // 2)]
items = [(2 * g, 2, 2, 0) for g in order]
encs = [m.pkg.Lc3Encoder.mixed(descs) for _ in range(2)]
decs = [m.pkg.Lc3Decoder.mixed(descs) for _ in range(2)]
cursor = [0] * n
m._mc_vs_items(encs, decs, descs, pcm, cursor, items, rng, "a stereo tick of %d channel-frames" % (2 * n))
assert np.array_equal(encs[0].state_save(), encs[1].state_save()) and np.array_equal(decs[0].state_save(), decs[1].state_save())
assert decs[0].plc_events() == decs[1].plc_events() > 0
# the same tick once more with ONE item at 400 bytes: the launch set's LDS is sized by its largest frame, which takes the pair kernels'
# workgroups beyond 64 KB.  That stream starts a new life and is held to fresh oracle objects, frame by frame
g400 = order[len(order) // 2]
c0 = 2 * g400
fs, us = descs[c0][0], descs[c0][1]
for h in (encs[0], decs[0]):
    h.reset([c0, c0 + 1])
items = [(2 * g, 2, 2, 400 if g == g400 else 0) for g in order]
x = [np.stack([pcm[c][cursor[c]:cursor[c] + 2] for c in (2 * g, 2 * g + 1)], axis=-1) for g in order]
nbs = [400 if g == g400 else descs[2 * g][2] for g in order]
at = order.index(g400)
b0, p0 = sum(4 * nb for nb in nbs[:at]), sum(a.size for a in x[:at])
st = m.cur_stream()
out = torch.full((sum(4 * nb for nb in nbs),), 0xA5, dtype=torch.uint8, device="cuda")
encs[0].encode_mixed_mc_items(items, m.dev(m._cat(x, np.int16)), out, stream=st)
torch.cuda.synchronize()
ref = np.zeros((2, 2, 400), np.uint8)
for ci in range(2):
    eo = m.O.Encoder(fs, us)
    for j in range(2):
        ref[j, ci] = eo.encode_frame(np.ascontiguousarray(x[at][j, :, ci]), 400)
assert np.array_equal(out.cpu().numpy()[b0:b0 + 1600].reshape(2, 2, 400), ref), "the 400-byte item's bytes differ from the oracle"
pcm_out = torch.full((sum(a.size for a in x),), 12345, dtype=torch.int16, device="cuda")
decs[0].decode_mixed_mc_items(items, out, pcm_out, stream=st)
torch.cuda.synchronize()
want = np.zeros(x[at].shape, np.int16)
for ci in range(2):
    do = m.O.Decoder(fs, us)
    for j in range(2):
        _, want[j, :, ci] = do.decode_frame(ref[j, ci])
assert np.array_equal(pcm_out.cpu().numpy()[p0:p0 + want.size].reshape(want.shape), want), "the 400-byte item's PCM differs from the oracle"
assert not bool((out == 0xA5).all()) and not bool((pcm_out == 12345).all())
for h in encs + decs:
    assert h.pair_timeouts() == 0
print("forms ok")
"""


def test_mc_items_every_kernel_form_in_a_fresh_process():
    """a short oracle-checked tick sequence, one stereo tick of two frames per item just above the full-batch threshold -- the pair packer
    and parser -- against the items call on twin handles, and that tick again with one item at 400 bytes against the oracle, per kernel
    form, each child under its own time limit; stops at the first child that fails"""
    threshold = ML._pc_threshold()
    for env in ML.FORMS:
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", _FORMS_CHILD, ROOT, str(threshold)], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "forms ok" in r.stdout, (env, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
