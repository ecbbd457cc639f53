"""lc3gpu_encode_vbr: a frame size per frame inside one batch launch -- the reference's per-call contract (nbits = 8 * buf_out.len(),
lc3_encoder.rs:65) for every channel and every frame at once.  Checked against oracle encoders fed frame by frame, against the uniform
call, and with the sizes a caller may get wrong (clamped and counted)."""
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
SENTINEL = 0xA5
# (fs, frame_us): the ten configurations the reference can encode
CONFIGS = [(fs, us) for us in (10000, 7500) for fs in (16000, 24000, 32000, 44100, 48000)]


def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch


def gpu_encode_vbr(enc, pcm, nb, slot, fill=SENTINEL):
    torch = torch_mod()
    S, T, _ = pcm.shape
    d_pcm = torch.from_numpy(np.ascontiguousarray(pcm)).cuda()
    d_nb = torch.from_numpy(np.ascontiguousarray(nb, np.uint16).view(np.int16)).cuda()
    d_out = torch.full((S, T, slot), fill, dtype=torch.uint8, device="cuda")
    enc.encode_vbr(d_pcm, d_out, d_nb, slot, T, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def gpu_encode(enc, pcm, nbytes):
    torch = torch_mod()
    S, T, _ = pcm.shape
    d_pcm = torch.from_numpy(np.ascontiguousarray(pcm)).cuda()
    d_out = torch.zeros((S, T, nbytes), dtype=torch.uint8, device="cuda")
    enc.encode(d_pcm, d_out, nbytes, T, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def oracle_vbr(oracles, pcm, nb, slot):
    """frames through per-stream oracle encoders (state carried in `oracles`), laid out as the sized call lays them out"""
    S, T, _ = pcm.shape
    out = np.full((S, T, slot), SENTINEL, np.uint8)
    for s in range(S):
        for t in range(T):
            n = int(min(max(int(nb[s, t]), 20), slot))
            out[s, t, :n] = oracles[s].encode_frame(pcm[s, t], n)
    return out


def _assert_same(got, want, what):
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, "%s: frames (stream, frame) differing from the oracle: %s" % (what, bad[:10].tolist())


def test_encode_vbr_against_the_oracle_with_state_across_calls():
    S, T, slot = 37, 24, 400  # 37 streams: a partial workgroup
    rng = np.random.default_rng(101)
    pcm = np.concatenate([synth.make_ltpf_pcm(480, 48000, n_frames=3 * T), synth.make_pcm(S - 3, 3 * T, 480, 48000, seed=57)], axis=0)
    enc = pkg.Lc3Encoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    oracles = [O.Encoder() for _ in range(S)]
    # sized call, uniform call, sized call: the state is carried through all three
    nb1 = rng.integers(20, 401, size=(S, T)).astype(np.uint16)
    got = gpu_encode_vbr(enc, pcm[:, :T], nb1, slot)
    _assert_same(got, oracle_vbr(oracles, pcm[:, :T], nb1, slot), "first sized call")
    got = gpu_encode(enc, pcm[:, T:2 * T], 97)
    for s in range(S):
        for t in range(T):
            assert np.array_equal(got[s, t], oracles[s].encode_frame(pcm[s, T + t], 97)), (s, t)
    nb3 = rng.integers(20, 401, size=(S, T)).astype(np.uint16)
    got = gpu_encode_vbr(enc, pcm[:, 2 * T:], nb3, slot)
    _assert_same(got, oracle_vbr(oracles, pcm[:, 2 * T:], nb3, slot), "second sized call")
    assert enc.size_clamps() == 0


@pytest.mark.parametrize("fs,us", CONFIGS)
def test_encode_vbr_every_configuration(fs, us):
    nf = {16000: 160, 24000: 240, 32000: 320, 44100: 480, 48000: 480}[fs] * (3 if us == 7500 else 4) // 4
    S, T, slot = 6, 7, 400
    rng = np.random.default_rng([fs, us])
    pcm = synth.make_pcm(S, T, nf, fs, seed=61)
    lo = 20
    nb = rng.integers(lo, slot + 1, size=(S, T)).astype(np.uint16)
    nb[:, ::3] = rng.integers(lo, 120, size=nb[:, ::3].shape)  # low rates too: LTPF on, weighting on
    enc = pkg.Lc3Encoder(S, us, fs)
    oracles = [O.Encoder(fs, us) for _ in range(S)]
    _assert_same(gpu_encode_vbr(enc, pcm, nb, slot), oracle_vbr(oracles, pcm, nb, slot), "%d Hz / %d us" % (fs, us))


def test_encode_vbr_ltpf_border_in_long_launches():
    # > 256 frames per stream in one launch, sizes alternating across 110 bytes (gain_ltpf_on) at different frames in the four streams of a
    # workgroup: the normalised-correlation shortcut and the phase's bit 8 both in play; the post-filter must switch on
    T, slot = 270, 160
    lt = synth.make_ltpf_pcm(480, 48000, n_frames=T)
    pcm = np.concatenate([lt, synth.make_pcm(3, T, 480, 48000, seed=71)], axis=0)
    S = pcm.shape[0]
    nb = np.full((S, T), 150, np.uint16)
    for s in range(S):
        period = 5 + s
        for t in range(T):
            if (t // period) % 3 == 0:
                nb[s, t] = 100 + (t % 10)  # 100 .. 109: the filter may switch on
    nb[:, 250:262] = 150  # a stretch where every stream keeps it off (the shortcut applies) ...
    nb[0, 262:] = 100  # ... then one stream drops below the border
    enc = pkg.Lc3Encoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    oracles = [O.Encoder() for _ in range(S)]
    got = gpu_encode_vbr(enc, pcm, nb, slot)
    want = oracle_vbr(oracles, pcm, nb, slot)
    _assert_same(got, want, "LTPF border")
    O.ltpf_transition_counts(reset=True)
    dec = O.Decoder()
    for t in range(T):
        dec.decode_frame(got[0, t, :int(nb[0, t])])
    assert sum(O.ltpf_transition_counts()[2:]) > 0, "the post-filter never switched on: the test material lost its point"


@pytest.mark.parametrize("S,T", [(16384, 4), (65536, 1)])
def test_encode_vbr_equal_sizes_match_the_uniform_call(S, T):
    pcm = synth.make_pcm_parallel(S, T, 480, 48000, seed=13)
    for n in (150, 60):
        a = pkg.Lc3Encoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
        b = pkg.Lc3Encoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
        uni = gpu_encode(a, pcm, n)
        vbr = gpu_encode_vbr(b, pcm, np.full((S, T), n, np.uint16), n)
        assert np.array_equal(uni, vbr), "%d x %d at %d bytes" % (S, T, n)


def test_encode_vbr_clamps_and_counts_out_of_range_sizes():
    S, T, slot = 4, 3, 120
    pcm = synth.make_pcm(S, T, 480, 48000, seed=83)
    nb = np.array([[0, 7, 19], [slot + 1, 60, 120], [20, 500, 110], [65535, 100, 1]], np.uint16)
    enc = pkg.Lc3Encoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    oracles = [O.Encoder() for _ in range(S)]
    _assert_same(gpu_encode_vbr(enc, pcm, nb, slot), oracle_vbr(oracles, pcm, nb, slot), "clamped sizes")
    assert enc.size_clamps() == 7
    gpu_encode_vbr(enc, synth.make_pcm(S, 1, 480, 48000, seed=84), np.full((S, 1), 3, np.uint16), slot)
    assert enc.size_clamps() == 11  # sticky


def test_encode_vbr_argument_errors():
    torch = torch_mod()
    L = pkg.load_library()
    S, T = 4, 2
    enc = pkg.Lc3Encoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    d_pcm = torch.zeros((S * T * 480 + 2,), dtype=torch.int16, device="cuda")
    d_nb = torch.full((S, T), 100, dtype=torch.int16, device="cuda")
    d_out = torch.zeros((S, T, 400), dtype=torch.uint8, device="cuda")
    p = lambda x: x.data_ptr()
    call = lambda pcm, out, nb, slot, t=T: L.lc3gpu_encode_vbr(enc._h, pcm, out, nb, slot, t, None)
    assert call(p(d_pcm), p(d_out), p(d_nb), 19) == -3
    assert call(p(d_pcm), p(d_out), p(d_nb), 401) == -3
    assert call(p(d_pcm), p(d_out), p(d_nb), 100, 0) == -3
    assert call(None, p(d_out), p(d_nb), 100) == -1
    assert call(p(d_pcm), None, p(d_nb), 100) == -1
    assert call(p(d_pcm), p(d_out), None, 100) == -1
    assert call(p(d_pcm) + 2, p(d_out), p(d_nb), 100) == -1  # PCM must be 4-byte aligned
    mixed = pkg.Lc3Encoder.mixed([(48000, 10000, 100), (16000, 10000, 40)])
    assert L.lc3gpu_encode_vbr(mixed._h, p(d_pcm), p(d_out), p(d_nb), 100, 1, None) == -1
    assert call(p(d_pcm), p(d_out), p(d_nb), 400) == 0
    torch.cuda.synchronize()


def gpu_decode_vbr(dec, data, nb, bad=None, nf=480):
    torch = torch_mod()
    S, T, slot = data.shape
    d_in = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    d_nb = torch.from_numpy(np.ascontiguousarray(nb, np.uint16).view(np.int16)).cuda()
    d_bad = torch.from_numpy(np.ascontiguousarray(bad, np.uint8)).cuda() if bad is not None else None
    d_pcm = torch.zeros((S, T, nf), dtype=torch.int16, device="cuda")
    dec.decode_vbr(d_in, d_nb, d_pcm, slot, T, stream=torch.cuda.current_stream().cuda_stream, d_bad_frame=d_bad)
    torch.cuda.synchronize()
    return d_pcm.cpu().numpy()


def oracle_decode_vbr(decoders, data, nb, bad=None):
    """per-stream oracle decoders fed frame by frame: an entry above the slot is an empty buf_in, a flagged frame is that frame with
    unparsable side information at its own size (the oracle has no external flag).  -> PCM, concealed frames"""
    S, T, slot = data.shape
    out = np.zeros((S, T, decoders[0].nf), np.int16)
    plc = 0
    for s in range(S):
        for t in range(T):
            n = int(nb[s, t])
            n = 0 if n > slot else n
            buf = data[s, t, :n].copy()
            if bad is not None and bad[s, t] and n > 0:
                buf[-1] |= 7
            _, out[s, t] = decoders[s].decode_frame(buf)
            plc += int(decoders[s].last_was_plc())
    return out, plc


def _sized_bytes(pcm, nb, slot, fs=48000, us=10000):
    return oracle_vbr([O.Encoder(fs, us) for _ in range(pcm.shape[0])], pcm, nb, slot)


def test_decode_vbr_against_the_oracle_with_empty_oversized_flagged_and_corrupt_frames():
    S, T, slot = 37, 24, 400
    rng = np.random.default_rng(202)
    pcm = np.concatenate([synth.make_ltpf_pcm(480, 48000, n_frames=2 * T), synth.make_pcm(S - 3, 2 * T, 480, 48000, seed=59)], axis=0)
    nb = rng.integers(20, 401, size=(S, 2 * T)).astype(np.uint16)
    data = _sized_bytes(pcm, nb, slot)
    nb_dec = nb.copy()
    nb_dec[rng.random((S, 2 * T)) < 0.05] = 0
    nb_dec[rng.random((S, 2 * T)) < 0.04] = rng.integers(slot + 1, 65536)
    bad = (rng.random((S, 2 * T)) < 0.05).astype(np.uint8)
    for s, t in zip(rng.integers(0, S, 40), rng.integers(0, 2 * T, 40)):
        data[s, t, rng.integers(0, max(1, int(nb[s, t])))] ^= 0x5A  # corrupted bytes, the same in both
    dec = pkg.Lc3Decoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    oracles = [O.Decoder() for _ in range(S)]
    # sized call, uniform call, sized call: the state is carried through all three
    got = gpu_decode_vbr(dec, data[:, :T], nb_dec[:, :T], bad[:, :T])
    want, plc1 = oracle_decode_vbr(oracles, data[:, :T], nb_dec[:, :T], bad[:, :T])
    assert np.abs(got.astype(np.int32) - want).max() <= 1 and np.array_equal(got, want)
    uni = O.encode_batch(synth.make_pcm(S, 3, 480, 48000, seed=60), 97)
    torch = torch_mod()
    d_pcm = torch.zeros((S, 3, 480), dtype=torch.int16, device="cuda")
    dec.decode(torch.from_numpy(uni).cuda(), d_pcm, 97, 3, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for s in range(S):
        for t in range(3):
            assert np.array_equal(d_pcm[s, t].cpu().numpy(), oracles[s].decode_frame(uni[s, t])[1]), (s, t)
    got = gpu_decode_vbr(dec, data[:, T:], nb_dec[:, T:], bad[:, T:])
    want, plc2 = oracle_decode_vbr(oracles, data[:, T:], nb_dec[:, T:], bad[:, T:])
    assert np.array_equal(got, want)
    assert plc1 + plc2 > 0 and dec.plc_events() == plc1 + plc2


@pytest.mark.parametrize("fs,us", CONFIGS)
def test_decode_vbr_every_configuration(fs, us):
    nf = {16000: 160, 24000: 240, 32000: 320, 44100: 480, 48000: 480}[fs] * (3 if us == 7500 else 4) // 4
    S, T, slot = 6, 7, 400
    rng = np.random.default_rng([fs, us, 2])
    pcm = synth.make_pcm(S, T, nf, fs, seed=62)
    nb = rng.integers(20, slot + 1, size=(S, T)).astype(np.uint16)
    nb[:, ::3] = rng.integers(20, 120, size=nb[:, ::3].shape)
    data = _sized_bytes(pcm, nb, slot, fs, us)
    nb[0, 3] = 0
    nb[1, 4] = slot + 7
    dec = pkg.Lc3Decoder(S, us, fs)
    want, plc = oracle_decode_vbr([O.Decoder(fs, us) for _ in range(S)], data, nb)
    assert np.array_equal(gpu_decode_vbr(dec, data, nb, nf=nf), want), "%d Hz / %d us" % (fs, us)
    assert dec.plc_events() == plc


@pytest.mark.parametrize("us", [10000, 7500])
def test_decode_vbr_8khz(us):
    # decode-only configuration: frames from the oracle's 8 kHz encoder (the specification switch), a size of its own per stream, and
    # empty / oversized entries in between
    nf, S, T, slot = 80 * us // 10000, 4, 6, 200
    pcm = synth.make_pcm(S, T, nf, 8000, seed=63)
    data = np.full((S, T, slot), SENTINEL, np.uint8)
    nb = np.zeros((S, T), np.uint16)
    for s, n in enumerate((20, 33, 61, 200)):
        data[s, :, :n] = O.encode_batch(pcm[s:s + 1], n, 8000, us, spec_flags=1)[0]
        nb[s] = n
    nb[0, 2] = 0
    nb[2, 4] = 999
    dec = pkg.Lc3Decoder(S, us, 8000)
    want, plc = oracle_decode_vbr([O.Decoder(8000, us) for _ in range(S)], data, nb)
    assert np.array_equal(gpu_decode_vbr(dec, data, nb, nf=nf), want)
    assert plc >= 2 and dec.plc_events() == plc


@pytest.mark.parametrize("S,T", [(16384, 4), (65536, 1)])
def test_decode_vbr_equal_sizes_match_the_uniform_call(S, T):
    torch = torch_mod()
    pcm = synth.make_pcm_parallel(S, T, 480, 48000, seed=14)
    for n in (150, 60):
        data = gpu_encode(pkg.Lc3Encoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000), pcm, n)
        bad = np.zeros((S, T), np.uint8)
        bad[::97, -1] = 1
        a = pkg.Lc3Decoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
        d_pcm = torch.zeros((S, T, 480), dtype=torch.int16, device="cuda")
        a.decode(torch.from_numpy(data).cuda(), d_pcm, n, T, stream=torch.cuda.current_stream().cuda_stream,
                 d_bad_frame=torch.from_numpy(bad).cuda())
        torch.cuda.synchronize()
        b = pkg.Lc3Decoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
        got = gpu_decode_vbr(b, data, np.full((S, T), n, np.uint16), bad)
        assert np.array_equal(d_pcm.cpu().numpy(), got), "%d x %d at %d bytes" % (S, T, n)
        assert a.plc_events() == b.plc_events()


def test_decode_vbr_argument_errors():
    torch = torch_mod()
    L = pkg.load_library()
    S, T = 4, 2
    dec = pkg.Lc3Decoder(S, pkg.FrameDuration.TenMs, pkg.SamplingFrequency.Hz48000)
    d_in = torch.zeros((S, T, 400), dtype=torch.uint8, device="cuda")
    d_nb = torch.full((S, T), 100, dtype=torch.int16, device="cuda")
    d_pcm = torch.zeros((S * T * 480 + 2,), dtype=torch.int16, device="cuda")
    p = lambda x: x.data_ptr()
    call = lambda i, nb, pcm, slot, t=T: L.lc3gpu_decode_vbr(dec._h, i, nb, None, pcm, slot, t, None)
    assert call(p(d_in), p(d_nb), p(d_pcm), 0) == -3
    assert call(p(d_in), p(d_nb), p(d_pcm), 401) == -3
    assert call(p(d_in), p(d_nb), p(d_pcm), 100, 0) == -3
    assert call(None, p(d_nb), p(d_pcm), 100) == -1
    assert call(p(d_in), None, p(d_pcm), 100) == -1
    assert call(p(d_in), p(d_nb), None, 100) == -1
    assert call(p(d_in), p(d_nb), p(d_pcm) + 2, 100) == -1
    mixed = pkg.Lc3Decoder.mixed([(48000, 10000, 100), (16000, 10000, 40)])
    assert L.lc3gpu_decode_vbr(mixed._h, p(d_in), p(d_nb), None, p(d_pcm), 100, 1, None) == -1
    assert call(p(d_in), p(d_nb), p(d_pcm), 400) == 0
    torch.cuda.synchronize()


_FORMS_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_vbr as m
import oracle_lib as O
pkg, synth = m.pkg, m.synth
FS, US = pkg.SamplingFrequency.Hz48000, pkg.FrameDuration.TenMs
rng = np.random.default_rng(5)
for S, T in [(1, 1), (3, 2), (5, 3), (2, 3)]:
    pcm = synth.make_pcm(S, T, 480, 48000, seed=S * 10 + T)
    nb = rng.integers(20, 201, size=(S, T)).astype(np.uint16)
    got = m.gpu_encode_vbr(pkg.Lc3Encoder(S, US, FS), pcm, nb, 200)
    m._assert_same(got, m.oracle_vbr([O.Encoder() for _ in range(S)], pcm, nb, 200), "encode %d x %d" % (S, T))
    nb[0, -1] = 0
    bad = np.zeros((S, T), np.uint8)
    bad[-1, 0] = 1
    want, _ = m.oracle_decode_vbr([O.Decoder() for _ in range(S)], got, nb, bad)
    assert np.array_equal(m.gpu_decode_vbr(pkg.Lc3Decoder(S, US, FS), got, nb, bad), want), "decode %d x %d" % (S, T)
S = 65536
pcm = synth.make_pcm_parallel(S, 1, 480, 48000, seed=3)
nb = rng.integers(20, 201, size=(S, 1)).astype(np.uint16)
got = m.gpu_encode_vbr(pkg.Lc3Encoder(S, US, FS), pcm, nb, 200)
idx = rng.choice(S, 300, replace=False)
m._assert_same(got[idx], m.oracle_vbr([O.Encoder() for _ in idx], pcm[idx], nb[idx], 200), "encode 65536 x 1 sample")
nb[::50] = 0
bad = np.zeros((S, 1), np.uint8)
bad[7::61] = 1
pcm_out = m.gpu_decode_vbr(pkg.Lc3Decoder(S, US, FS), got, nb, bad)
want, _ = m.oracle_decode_vbr([O.Decoder() for _ in idx], got[idx], nb[idx], bad[idx])
assert np.array_equal(pcm_out[idx], want), "decode 65536 x 1 sample"
print("forms ok")
"""


@pytest.mark.parametrize("env", [{"LC3GPU_PREP_SYMBOLS": "0"}, {"LC3GPU_PREP_SYMBOLS": "1"}, {"LC3GPU_PREP_SYMBOLS": "2"},
                                 {"LC3GPU_RECON": "lane"}, {"LC3GPU_RECON": "late"}, {"LC3GPU_RECON": "wave"}, {}])
def test_vbr_every_kernel_form_in_a_fresh_process(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _FORMS_CHILD, ROOT], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "forms ok" in r.stdout, (env, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
