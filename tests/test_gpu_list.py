"""lc3gpu_encode_list / lc3gpu_decode_list, per-channel resets and per-channel state blobs on the GPU: identical bytes and identical PCM
throughout, against one oracle encoder / decoder per channel LIFE (a reset channel gets a new oracle object, as the reference's caller
builds a new EncoderChannel / DecoderChannel) and against the uniform / range calls on twin handles."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("lc3-codec_amd")
synth = importlib.import_module("lc3-codec_amd.synth")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, US = pkg.SamplingFrequency.Hz48000, pkg.FrameDuration.TenMs
# (fs, frame_us, nbytes): the ten configurations the reference can encode, at sizes where the post-filter may switch on
ENC_CONFIGS = [(16000, 10000, 40), (24000, 10000, 60), (32000, 10000, 80), (44100, 10000, 100), (48000, 10000, 100),
               (16000, 7500, 30), (24000, 7500, 45), (32000, 7500, 60), (44100, 7500, 75), (48000, 7500, 80)]
EINVAL, ECHANNEL, ELENGTH = -1, -2, -3


def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch


def dev(a):
    return torch_mod().from_numpy(np.ascontiguousarray(a)).cuda()


def cur_stream():
    return torch_mod().cuda.current_stream().cuda_stream


class Server:
    """n_ch channels of one configuration on an encoder and a decoder handle, the oracle objects of their current lives beside them.
    A channel's PCM runs on through its resets (a new stream takes the channel over mid-signal)."""

    def __init__(self, fs, us, nbytes, n_ch, total_frames, seed, encode=True):
        self.fs, self.us, self.nbytes, self.n_ch = fs, us, nbytes, n_ch
        self.nf = pkg.Lc3Config(fs, us).nf
        self.material = np.concatenate([synth.make_ltpf_pcm(self.nf, fs, n_frames=total_frames),
                                        synth.make_pcm(n_ch - 3, total_frames, self.nf, fs, seed=seed)], axis=0)
        self.cursor = [0] * n_ch
        self.enc = pkg.Lc3Encoder(n_ch, us, fs) if encode else None
        self.dec = pkg.Lc3Decoder(n_ch, us, fs)
        self.enc_or = [O.Encoder(fs, us) for _ in range(n_ch)] if encode else None
        self.dec_or = [O.Decoder(fs, us) for _ in range(n_ch)]
        self.plc = [0] * n_ch  # frames concealed in the channel's current decoder life
        # without an encoder (8 kHz: the reference cannot encode it) the frames come from the oracle's batch encoder, one stream per channel
        self.frames = None if encode else O.encode_batch(self.material, nbytes, fs, us)
        self.rng = np.random.default_rng(seed)

    def reset_enc(self, chs):
        self.enc.reset(chs)
        for c in chs:
            self.enc_or[c] = O.Encoder(self.fs, self.us)

    def reset_dec(self, chs):
        self.dec.reset(chs)
        for c in chs:
            self.dec_or[c] = O.Decoder(self.fs, self.us)
            self.plc[c] = 0

    def step(self, ch, T, how="list", what=""):
        """T frames of the channels `ch` through the encoder and the decoder by the call `how` (list, uniform, range, frame)"""
        torch = torch_mod()
        n, nbytes, nf, rng = len(ch), self.nbytes, self.nf, self.rng
        pcm = np.stack([self.material[c, self.cursor[c]:self.cursor[c] + T] for c in ch])
        if self.enc is not None:
            ref = np.stack([np.stack([self.enc_or[c].encode_frame(pcm[i, j], nbytes) for j in range(T)]) for i, c in enumerate(ch)])
            d_pcm, d_out = dev(pcm), torch.full((n, T, nbytes), 0xA5, dtype=torch.uint8, device="cuda")
            if how == "list":
                self.enc.encode_list(ch, d_pcm, d_out, nbytes, T, stream=cur_stream())
            elif how == "uniform":
                assert list(ch) == list(range(self.n_ch))
                self.enc.encode(d_pcm, d_out, nbytes, T, stream=cur_stream())
            elif how == "range":
                assert list(ch) == list(range(ch[0], ch[0] + n))
                self.enc.encode(d_pcm, d_out, nbytes, T, stream=cur_stream(), first_channel=ch[0], n_channels=n)
            else:
                assert T == 1
                got = np.zeros((n, 1, nbytes), np.uint8)
                for i, c in enumerate(ch):
                    self.enc.encode_frame(c, pcm[i, 0], got[i, 0])
                d_out = dev(got)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            bad = np.argwhere((got != ref).any(axis=2))
            assert bad.size == 0, "%s encode (%s): (list position, frame) differing from the oracle: %s, channels %s" % (what, how, bad[:10].tolist(), list(ch))
        else:
            ref = np.stack([self.frames[c, self.cursor[c]:self.cursor[c] + T] for c in ch])
        # the decoder's input: some frames corrupt, some flagged (the *_frame call has no flag)
        xor = np.zeros((n, T, nbytes), np.uint8)
        for i, j in np.argwhere(rng.random((n, T)) < 0.12):
            xor[i, j, rng.integers(0, nbytes, 3)] = rng.integers(1, 256, 3)
        data = ref ^ xor
        flags = (rng.random((n, T)) < (0.0 if how == "frame" else 0.1)).astype(np.uint8)
        want = np.zeros((n, T, nf), np.int16)
        for i, c in enumerate(ch):
            for j in range(T):
                buf = data[i, j].copy()
                if flags[i, j]:
                    buf[-2:] = 0xFF  # (the oracle has no external flag: unparsable side information at the frame's own size)
                _, want[i, j] = self.dec_or[c].decode_frame(buf)
                assert not flags[i, j] or self.dec_or[c].last_was_plc()
                self.plc[c] += int(self.dec_or[c].last_was_plc())
            self.cursor[c] += T
        d_in, d_bad, d_pcm = dev(data), dev(flags), torch.full((n, T, nf), 12345, dtype=torch.int16, device="cuda")
        if how == "list":
            self.dec.decode_list(ch, d_in, d_pcm, nbytes, T, stream=cur_stream(), d_bad_frame=d_bad)
        elif how == "uniform":
            self.dec.decode(d_in, d_pcm, nbytes, T, stream=cur_stream(), d_bad_frame=d_bad)
        elif how == "range":
            self.dec.decode(d_in, d_pcm, nbytes, T, stream=cur_stream(), d_bad_frame=d_bad, first_channel=ch[0], n_channels=n)
        else:
            got = np.zeros((n, 1, nf), np.int16)
            for i, c in enumerate(ch):
                self.dec.decode_frame(16, c, data[i, 0], got[i, 0])
            d_pcm = dev(got)
        torch.cuda.synchronize()
        got = d_pcm.cpu().numpy()
        bad = np.argwhere((got != want).any(axis=2))
        assert bad.size == 0, "%s decode (%s): (list position, frame) differing from the oracle: %s, channels %s" % (what, how, bad[:10].tolist(), list(ch))


def _random_ticks(sv, n_ticks, rng, calls=("list",), sizes=(1, 2, 5)):
    n_ch = sv.n_ch
    for k in range(n_ticks):
        # single channels end and start between the ticks
        if k and sv.enc is not None:
            sv.reset_enc([int(c) for c in rng.choice(n_ch, int(rng.integers(0, 4)), replace=False)])
        if k:
            sv.reset_dec([int(c) for c in rng.choice(n_ch, int(rng.integers(0, 4)), replace=False)])
        how = calls[int(rng.integers(0, len(calls)))] if k else "list"
        T = int(sizes[k % len(sizes)])
        if how == "uniform":
            ch = list(range(n_ch))
        elif how == "range":
            a = int(rng.integers(0, n_ch - 1))
            ch = list(range(a, int(rng.integers(a + 1, n_ch + 1))))
        elif how == "frame":
            ch, T = [int(c) for c in rng.choice(n_ch, 3, replace=False)], 1
        else:
            ch = [int(c) for c in rng.choice(n_ch, int(rng.integers(1, n_ch + 1)), replace=False)]
        sv.step(ch, T, how, "tick %d" % k)


def test_server_ticks_against_the_oracle():
    n_ch, n_ticks = 40, 34
    rng = np.random.default_rng(404)
    sv = Server(48000, 10000, 100, n_ch, 5 * n_ticks + 8, seed=17)
    # a first stretch on the LTPF material's channels so that their filters are on when they are reset
    sv.step([2, 0, 1, 17], 5, "list", "warm-up")
    sv.reset_enc([0, 2])
    sv.reset_dec([1, 2])
    sv.step([9, 2, 1, 0, 30, 31, 32, 33, 5], 1, "list", "fresh beside carried")
    _random_ticks(sv, n_ticks, rng, calls=("list", "list", "list", "list", "uniform", "range", "frame"))
    assert sv.dec.plc_events() == sum(sv.plc), "PLC count over the channels' current lives"
    assert sum(sv.plc) > 0
    assert sv.enc.pair_timeouts() == 0 and sv.dec.pair_timeouts() == 0


@pytest.mark.parametrize("fs,us,nbytes", ENC_CONFIGS)
def test_list_ticks_every_configuration(fs, us, nbytes):
    sv = Server(fs, us, nbytes, 9, 40, seed=fs // 100 + us // 100)
    _random_ticks(sv, 7, np.random.default_rng([fs, us]))
    assert sv.dec.plc_events() == sum(sv.plc)


@pytest.mark.parametrize("us", [10000, 7500])
def test_decode_list_ticks_8khz(us):
    sv = Server(8000, us, 30, 9, 40, seed=us // 100, encode=False)
    _random_ticks(sv, 7, np.random.default_rng([8000, us]))
    assert sv.dec.plc_events() == sum(sv.plc)


_BIG = {}


def _big_pcm():
    if "pcm" not in _BIG:
        _BIG["pcm"] = synth.make_pcm_parallel(65536, 2, 480, 48000, seed=9)
    return _BIG["pcm"]


def _list_vs_uniform(S, T, pcm, nbytes=150, nf=480):
    """list = arange against the uniform call on a twin handle, and a random permutation of all channels against the uniform call with the
    buffers permuted the same way; two calls each (fresh, then carried), encoder and decoder.  pcm int16[S][2 * T][nf]"""
    torch = torch_mod()
    rng = np.random.default_rng(S)
    perm = rng.permutation(S).astype(np.int32)
    d_perm = dev(perm.astype(np.int64))
    enc_u, enc_a, enc_p = (pkg.Lc3Encoder(S, US, FS) for _ in range(3))
    dec_u, dec_a, dec_p = (pkg.Lc3Decoder(S, US, FS) for _ in range(3))
    st = cur_stream()
    for half in range(2):
        d_pcm = dev(pcm[:, half * T:(half + 1) * T])
        outs = [torch.zeros((S, T, nbytes), dtype=torch.uint8, device="cuda") for _ in range(3)]
        enc_u.encode(d_pcm, outs[0], nbytes, T, stream=st)
        enc_a.encode_list(np.arange(S), d_pcm, outs[1], nbytes, T, stream=st)
        d_pcm_p = d_pcm[d_perm].contiguous()  # item i = the frames of channel perm[i]
        enc_p.encode_list(perm, d_pcm_p, outs[2], nbytes, T, stream=st)
        torch.cuda.synchronize()
        assert torch.equal(outs[1], outs[0]), "encode_list(arange) differs from encode (call %d)" % half
        assert torch.equal(outs[2], outs[0][d_perm]), "encode_list(permutation) differs from encode (call %d)" % half
        flags = dev((rng.random((S, T)) < 0.02).astype(np.uint8))
        pcms = [torch.zeros((S, T, nf), dtype=torch.int16, device="cuda") for _ in range(3)]
        dec_u.decode(outs[0], pcms[0], nbytes, T, stream=st, d_bad_frame=flags)
        dec_a.decode_list(np.arange(S), outs[0], pcms[1], nbytes, T, stream=st, d_bad_frame=flags)
        dec_p.decode_list(perm, outs[0][d_perm].contiguous(), pcms[2], nbytes, T, stream=st, d_bad_frame=flags[d_perm].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(pcms[1], pcms[0]), "decode_list(arange) differs from decode (call %d)" % half
        assert torch.equal(pcms[2], pcms[0][d_perm]), "decode_list(permutation) differs from decode (call %d)" % half
    assert dec_a.plc_events() == dec_u.plc_events() == dec_p.plc_events() > 0
    for h in (enc_a, enc_p, dec_a, dec_p):
        assert h.pair_timeouts() == 0
    # a state saved under the permuted list is the uniform handle's
    assert np.array_equal(enc_p.state_save(), enc_u.state_save())
    assert np.array_equal(dec_p.state_save(), dec_u.state_save())


@pytest.mark.parametrize("S,T", [(65536, 1), (16384, 4)])
def test_list_equals_the_uniform_call_at_size(S, T):
    """150 bytes, 65 536 frames per call: full batches, so the producer / consumer pair kernels run under a list call"""
    _list_vs_uniform(S, T, _big_pcm().reshape(S, 2 * T, 480))


def test_contiguous_list_equals_the_range_call():
    torch = torch_mod()
    S, T, nbytes, nf = 64, 3, 100, 480
    pcm = synth.make_pcm(S, 2 * T, nf, 48000, seed=31)
    enc_r, enc_l = pkg.Lc3Encoder(S, US, FS), pkg.Lc3Encoder(S, US, FS)
    dec_r, dec_l = pkg.Lc3Decoder(S, US, FS), pkg.Lc3Decoder(S, US, FS)
    first, n = 13, 30
    for half in range(2):
        d_pcm = dev(pcm[first:first + n, half * T:(half + 1) * T])
        a, b = (torch.zeros((n, T, nbytes), dtype=torch.uint8, device="cuda") for _ in range(2))
        enc_r.encode(d_pcm, a, nbytes, T, stream=cur_stream(), first_channel=first, n_channels=n)
        enc_l.encode_list(range(first, first + n), d_pcm, b, nbytes, T, stream=cur_stream())
        pa, pb = (torch.zeros((n, T, nf), dtype=torch.int16, device="cuda") for _ in range(2))
        dec_r.decode(a, pa, nbytes, T, stream=cur_stream(), first_channel=first, n_channels=n)
        dec_l.decode_list(range(first, first + n), b, pb, nbytes, T, stream=cur_stream())
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(pa, pb), half
    assert np.array_equal(enc_r.state_save(), enc_l.state_save())
    assert np.array_equal(dec_r.state_save(), dec_l.state_save())


def test_untouched_means_untouched():
    torch = torch_mod()
    S, T, nbytes, nf = 64, 2, 100, 480
    rng = np.random.default_rng(77)
    pcm = synth.make_pcm(S, 3 * T, nf, 48000, seed=41)
    enc, dec = pkg.Lc3Encoder(S, US, FS), pkg.Lc3Decoder(S, US, FS)
    d_out = torch.zeros((S, T, nbytes), dtype=torch.uint8, device="cuda")
    d_pcm_out = torch.zeros((S, T, nf), dtype=torch.int16, device="cuda")
    enc.encode(dev(pcm[:, :T]), d_out, nbytes, T, stream=cur_stream())
    flags = np.zeros((S, T), np.uint8)
    flags[::5, 0] = 1  # PLC counts on some channels
    dec.decode(d_out, d_pcm_out, nbytes, T, stream=cur_stream(), d_bad_frame=dev(flags))
    torch.cuda.synchronize()
    half = np.sort(rng.choice(S, S // 2, replace=False)).astype(np.int32)
    rest = np.setdiff1d(np.arange(S), half).astype(np.int32)
    order = rng.permutation(half)
    enc_before, dec_before = enc.state_save(rest), dec.state_save(rest)
    whole_enc, whole_dec = enc.state_save(), dec.state_save()
    # (a slice of the whole-handle save IS the per-channel save)
    per_e, per_d = whole_enc.size // S, whole_dec.size // S
    assert np.array_equal(enc_before.reshape(-1, per_e), whole_enc.reshape(S, per_e)[rest])
    assert np.array_equal(dec_before.reshape(-1, per_d), whole_dec.reshape(S, per_d)[rest])
    plc_before = dec.plc_events()
    n = order.size
    d_out2 = torch.zeros((n, T, nbytes), dtype=torch.uint8, device="cuda")
    enc.reset([int(order[0]), int(order[3])])
    dec.reset([int(order[1])])
    enc.encode_list(order, dev(pcm[order, T:2 * T]), d_out2, nbytes, T, stream=cur_stream())
    bad2 = np.ones((n, T), np.uint8)
    dec.decode_list(order, d_out2, torch.zeros((n, T, nf), dtype=torch.int16, device="cuda"), nbytes, T, stream=cur_stream(), d_bad_frame=dev(bad2))
    torch.cuda.synchronize()
    assert np.array_equal(enc.state_save(rest), enc_before), "encoder channels that were not listed changed"
    assert np.array_equal(dec.state_save(rest), dec_before), "decoder channels that were not listed changed"
    lost = int(flags[order[1]].sum())  # the reset channel's earlier count is gone with its reset
    assert dec.plc_events() == plc_before - lost + n * T
    assert not np.array_equal(enc.state_save(half), whole_enc.reshape(S, per_e)[half].reshape(-1))


def test_argument_errors_launch_nothing_and_advance_nothing():
    torch = torch_mod()
    L = pkg.load_library()
    S, nbytes, nf = 8, 100, 480
    pcm = synth.make_pcm(S, 3, nf, 48000, seed=51)
    enc, dec = pkg.Lc3Encoder(S, US, FS), pkg.Lc3Decoder(S, US, FS)
    enc_or, dec_or = [O.Encoder() for _ in range(S)], [O.Decoder() for _ in range(S)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    cp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def valid(t, ch):
        d_out = torch.zeros((len(ch), 1, nbytes), dtype=torch.uint8, device="cuda")
        d_pcm_out = torch.zeros((len(ch), 1, nf), dtype=torch.int16, device="cuda")
        enc.encode_list(ch, dev(pcm[ch, t:t + 1]), d_out, nbytes, 1, stream=cur_stream())
        dec.decode_list(ch, d_out, d_pcm_out, nbytes, 1, stream=cur_stream())
        torch.cuda.synchronize()
        got, got_pcm = d_out.cpu().numpy(), d_pcm_out.cpu().numpy()
        for i, c in enumerate(ch):
            ref = enc_or[c].encode_frame(pcm[c, t], nbytes)
            assert np.array_equal(got[i, 0], ref), (t, c)
            assert np.array_equal(got_pcm[i, 0], dec_or[c].decode_frame(ref)[1]), (t, c)

    valid(0, [5, 1, 6, 2])
    ok = np.array([3, 1, 2, 6], np.int32)
    d_pcm = dev(pcm[ok, 1:2])
    d_out = torch.full((4, 1, nbytes), 0xA5, dtype=torch.uint8, device="cuda")
    d_pcm_out = torch.full((4, 1, nf), 12345, dtype=torch.int16, device="cuda")
    st = ctypes.c_void_p(cur_stream())
    E = lambda ch, n, a, b, nb=nbytes, T=1, h=None: L.lc3gpu_encode_list(h or enc._h, ch, n, a, b, nb, T, st)
    D = lambda ch, n, a, b, nb=nbytes, T=1, h=None: L.lc3gpu_decode_list(h or dec._h, ch, n, a, None, b, nb, T, st)
    for call, a, b in ((E, p(d_pcm), p(d_out)), (D, p(d_out), p(d_pcm_out))):
        assert call(cp(np.array([3, 1, 8, 6], np.int32)), 4, a, b) == ECHANNEL
        assert call(cp(np.array([3, -1, 2, 6], np.int32)), 4, a, b) == ECHANNEL
        assert call(cp(np.array([3, 1, 3, 6], np.int32)), 4, a, b) == ECHANNEL  # a channel named twice
        assert call(None, 4, a, b) == EINVAL
        assert call(cp(ok), 4, None, b) == EINVAL
        assert call(cp(ok), 4, a, None) == EINVAL
        assert call(cp(ok), -1, a, b) == EINVAL
        assert call(cp(ok), 4, a, b, T=0) == ELENGTH
        assert call(cp(ok), 4, a, b, nb=401) == ELENGTH
        assert call(cp(ok), 0, a, b) == 0  # an empty list launches nothing
    assert E(cp(ok), 4, p(d_pcm), p(d_out), nb=19) == ELENGTH
    assert D(cp(ok), 4, p(d_out), p(d_pcm_out), nb=0) == ELENGTH
    assert E(cp(ok), 4, ctypes.c_void_p(d_pcm.data_ptr() + 2), p(d_out)) == EINVAL  # misaligned PCM
    assert D(cp(ok), 4, p(d_out), ctypes.c_void_p(d_pcm_out.data_ptr() + 2)) == EINVAL
    menc = pkg.Lc3Encoder.mixed([(48000, 10000, 100), (16000, 10000, 40)])
    mdec = pkg.Lc3Decoder.mixed([(48000, 10000, 100), (16000, 10000, 40)])
    one = np.array([0], np.int32)
    assert E(cp(one), 1, p(d_pcm), p(d_out), h=menc._h) == EINVAL
    assert D(cp(one), 1, p(d_out), p(d_pcm_out), h=mdec._h) == EINVAL
    # reset_channels: out of range / null / negative; a channel named twice is harmless
    for f, h in ((L.lc3gpu_encoder_reset_channels, enc._h), (L.lc3gpu_decoder_reset_channels, dec._h)):
        assert f(h, cp(np.array([0, 8], np.int32)), 2) == ECHANNEL
        assert f(h, None, 2) == EINVAL
        assert f(h, cp(ok), -1) == EINVAL
    # a bound handle takes the call on its bound stream only
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    enc.bind_stream(s1.cuda_stream)
    dec.bind_stream(s1.cuda_stream)
    s2p = ctypes.c_void_p(s2.cuda_stream)
    assert L.lc3gpu_encode_list(enc._h, cp(ok), 4, p(d_pcm), p(d_out), nbytes, 1, s2p) == EINVAL
    assert L.lc3gpu_decode_list(dec._h, cp(ok), 4, p(d_out), None, p(d_pcm_out), nbytes, 1, s2p) == EINVAL
    enc.bind_stream(s1.cuda_stream, bind=False)
    dec.bind_stream(s1.cuda_stream, bind=False)
    torch.cuda.synchronize()
    assert bool((d_out == 0xA5).all()) and bool((d_pcm_out == 12345).all()), "a refused call wrote to its output"
    # nothing was launched, advanced or reset: the next valid calls give the oracle's bytes, on channels the refused calls named too
    valid(1, [3, 1, 2, 6, 0])
    valid(2, [7, 6, 5, 4, 3, 2, 1, 0])


def test_per_channel_blobs_move_streams_between_handles():
    torch = torch_mod()
    nbytes, nf, T = 100, 480, 3
    lt = synth.make_ltpf_pcm(nf, 48000, n_frames=4 * T)  # post-filter memories in play
    a, b, c, d = 1, 6, 4, 0
    enc1, enc2 = pkg.Lc3Encoder(8, US, FS), pkg.Lc3Encoder(5, US, FS)
    dec1, dec2 = pkg.Lc3Decoder(8, US, FS), pkg.Lc3Decoder(5, US, FS)

    def run(enc, dec, ch, t0):
        d_out = torch.zeros((len(ch), T, nbytes), dtype=torch.uint8, device="cuda")
        d_pcm = torch.zeros((len(ch), T, nf), dtype=torch.int16, device="cuda")
        enc.encode_list(ch, dev(lt[:2, t0:t0 + T]), d_out, nbytes, T, stream=cur_stream())
        dec.decode_list(ch, d_out, d_pcm, nbytes, T, stream=cur_stream())
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), d_pcm.cpu().numpy()

    run(enc1, dec1, [a, b], 0)
    run(enc1, dec1, [a, b], T)
    run(enc2, dec2, [d, c], 0)  # the target's channels hold something else
    enc2.state_load(enc1.state_save([a, b]), [c, d])
    dec2.state_load(dec1.state_save([a, b]), [c, d])
    for t0 in (2 * T, 3 * T):
        b1, p1 = run(enc1, dec1, [a, b], t0)
        b2, p2 = run(enc2, dec2, [c, d], t0)
        assert np.array_equal(b1, b2) and np.array_equal(p1, p2), t0
    # a slice of a whole-handle save loads through the per-channel call
    per = enc1.state_save().size // 8
    enc2.state_load(enc1.state_save().reshape(8, per)[[b]].reshape(-1), [2])
    assert np.array_equal(enc2.state_save([2]), enc1.state_save([b]))
    # a blob of another configuration (or of the other side) is refused and no channel of the target changes
    other = pkg.Lc3Encoder(2, pkg.FrameDuration.SevenPointFiveMs, FS)
    before = enc2.state_save()
    mixed_blobs = np.concatenate([enc1.state_save([a]), other.state_save([0])[:per]])
    for blobs in (mixed_blobs, dec1.state_save([a, b])[:2 * per]):
        with pytest.raises(pkg.Lc3EncoderError) as ei:
            enc2.state_load(blobs, [0, 1])
        assert ei.value.code == EINVAL
    assert np.array_equal(enc2.state_save(), before)
    dbefore = dec2.state_save()
    dper = dbefore.size // 5
    odec = pkg.Lc3Decoder(2, pkg.FrameDuration.SevenPointFiveMs, FS)
    with pytest.raises(pkg.Lc3DecoderError) as ei:
        dec2.state_load(np.concatenate([dec1.state_save([a]), odec.state_save([1])[:dper]]), [3, 4])
    assert ei.value.code == EINVAL
    assert np.array_equal(dec2.state_save(), dbefore)
    L = pkg.load_library()
    buf = np.zeros(per, np.uint8)
    cp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert L.lc3gpu_encoder_state_save_channels(enc2._h, cp(np.array([5], np.int32)), 1, cp(buf), per) == ECHANNEL
    assert L.lc3gpu_encoder_state_save_channels(enc2._h, cp(np.array([1], np.int32)), 1, cp(buf), per - 16) == ELENGTH


_FORMS_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_list as m
for fs, us, nbytes in [(48000, 10000, 100), (32000, 7500, 60)]:
    sv = m.Server(fs, us, nbytes, 9, 40, seed=3)
    m._random_ticks(sv, 6, np.random.default_rng(8))
    assert sv.dec.plc_events() == sum(sv.plc)
# a launch large enough for the packer / parser forms of full batches (above 16 384 frames)
S = 20480
m._list_vs_uniform(S, 1, m.synth.make_pcm_parallel(S, 2, 480, 48000, seed=5))
print("forms ok")
"""
FORMS = [{"LC3GPU_RECON": "lane"}, {"LC3GPU_RECON": "late"}, {"LC3GPU_RECON": "wave"}, {"LC3GPU_PACK_PC": "0"}, {"LC3GPU_PARSE_PC": "0"},
         {"LC3GPU_PREP_SYMBOLS": "0"}, {"LC3GPU_PREP_SYMBOLS": "1"}, {"LC3GPU_PREP_SYMBOLS": "2"}]


def test_list_every_kernel_form_in_a_fresh_process():
    """one short tick sequence per kernel form, each child under its own time limit; stops at the first child that fails"""
    for env in FORMS:
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", _FORMS_CHILD, ROOT], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "forms ok" in r.stdout, (env, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
