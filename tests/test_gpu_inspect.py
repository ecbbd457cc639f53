"""lc3gpu_inspect on the GPU: every record against the oracle's stage entry points (lc3o_dec_side_info + lc3o_dec_arith) in all 12
configurations and on a full 65 536-frame batch, and the call's contract with the decoder -- status != 0 exactly for the frames that
lc3gpu_decode / lc3gpu_decode_vbr conceal (per frame against an oracle decoder fed frame by frame, and in count against the handles'
PLC counters).  Also: batch sizes around the workgroup size, ordering on the caller's stream, a process that created no codec handle, and
argument errors."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import inspect_lib as I
import oracle_lib as O

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("lc3-codec_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch


def _dev(a, dtype=None):
    torch = torch_mod()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def gpu_inspect(fs, us, data, nb=None, bad=None):
    torch = torch_mod()
    data = np.ascontiguousarray(data, np.uint8)
    n, slot = data.shape
    d_info = torch.full((max(n, 1), I.WORDS), -7, dtype=torch.int32, device="cuda")
    pkg.inspect(us, fs, _dev(data), d_info, slot, n, d_nbytes=None if nb is None else _dev(np.asarray(nb, np.uint16)),
                d_bad_frame=None if bad is None else _dev(np.asarray(bad, np.uint8)), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_info.cpu().numpy()[:n]


def _assert_records(got, ref, what):
    diff = np.nonzero((got != ref).any(1))[0]
    assert len(diff) == 0, "%s: %d records differ from the oracle; first frame %d\noracle %s\ngpu    %s" % (
        what, len(diff), diff[0], ref[diff[0]].tolist(), got[diff[0]].tolist())


def _decode_plc(fs, us, data, bad, streams, nb=None):
    """PLC events of one lc3gpu_decode (nb None) or lc3gpu_decode_vbr call over data uint8[streams * T][slot] (planar) on a fresh handle"""
    torch = torch_mod()
    n, slot = data.shape
    T = n // streams
    cfg = I.config(fs, us)
    dec = pkg.Lc3Decoder(streams, us, fs)
    d_pcm = torch.zeros((streams, T, cfg.nf), dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    d_bad = None if bad is None else _dev(np.asarray(bad, np.uint8))
    before = dec.plc_events()
    if nb is None:
        dec.decode(_dev(data), d_pcm, slot, T, stream=st, d_bad_frame=d_bad)
    else:
        dec.decode_vbr(_dev(data), _dev(np.asarray(nb, np.uint16)), d_pcm, slot, T, stream=st, d_bad_frame=d_bad)
    torch.cuda.synchronize()
    plc = dec.plc_events() - before
    dec.close()
    return plc


@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_every_configuration_against_the_oracle_and_the_decoder(fs, us):
    data, nb, bad = I.config_corpus(fs, us, np.random.default_rng(fs * 7 + us))
    ref = I.oracle_records(fs, us, data, nb, bad)
    got = gpu_inspect(fs, us, data, nb, bad)
    _assert_records(got, ref, "%d Hz / %d us" % (fs, us))
    # the decoder contract, sized: one stream through lc3gpu_decode_vbr
    lost = got[:, 0] != 0
    assert np.array_equal(lost, I.oracle_plc(fs, us, data, nb, bad))
    assert _decode_plc(fs, us, data, bad, 1, nb) == lost.sum()
    # uniform (every frame slot_bytes long, d_nbytes NULL): the 400-byte part of the corpus, one stream through lc3gpu_decode
    tail = data[-48:]
    got = gpu_inspect(fs, us, tail, None, bad[-48:])
    _assert_records(got, I.oracle_records(fs, us, tail, None, bad[-48:]), "%d Hz / %d us, d_nbytes NULL" % (fs, us))
    assert _decode_plc(fs, us, tail, bad[-48:], 1) == (got[:, 0] != 0).sum()


@pytest.fixture(scope="module")
def big_batch():
    """65 536 frames of 48 kHz / 10 ms / 150 bytes from 64 streams, about 10 % of them damaged (flips, random tails; truncations in the
    sizes), 1 % flagged"""
    S, T = 64, 1024
    pcm = importlib.import_module("lc3-codec_amd.synth").make_pcm(S, T, 480, 48000, seed=3)
    clean = O.encode_batch(pcm, 150, threads=16).reshape(S * T, 150)
    rng = np.random.default_rng(65536)
    data, sizes = I.damage(clean, rng, frac=0.10)
    bad = (rng.random(S * T) < 0.01).astype(np.uint8)
    return S, data, sizes.astype(np.uint16), bad


def test_full_batch_uniform_against_the_oracle_and_lc3gpu_decode(big_batch):
    S, data, _, bad = big_batch
    got = gpu_inspect(48000, 10000, data, None, bad)
    _assert_records(got, I.oracle_records(48000, 10000, data, None, bad), "65 536 frames")
    lost = got[:, 0] != 0
    assert 0.02 < lost.mean() < 0.2
    assert np.array_equal(lost, I.oracle_plc(48000, 10000, data, None, bad, streams=S))
    assert _decode_plc(48000, 10000, data, bad, S) == lost.sum()


def test_full_batch_sized_against_the_oracle_and_lc3gpu_decode_vbr(big_batch):
    S, data, nb, bad = big_batch
    got = gpu_inspect(48000, 10000, data, nb, bad)
    _assert_records(got, I.oracle_records(48000, 10000, data, nb, bad), "65 536 frames, sized")
    lost = got[:, 0] != 0
    assert np.array_equal(lost, I.oracle_plc(48000, 10000, data, nb, bad, streams=S))
    assert _decode_plc(48000, 10000, data, bad, S, nb) == lost.sum()


@pytest.mark.parametrize("n", [1, 63, 257])
def test_batch_sizes(n):
    rng = np.random.default_rng(n)
    clean = I.clean_frames(32000, 7500, 80, n, seed=n)
    data, nb = I.damage(clean, rng, frac=0.3)
    for sizes in (None, nb.astype(np.uint16)):
        _assert_records(gpu_inspect(32000, 7500, data, sizes), I.oracle_records(32000, 7500, data, sizes), "n_frames %d" % n)
    # random bytes at an odd slot size (unaligned slots)
    data = I.random_frames(n, 77, rng)
    _assert_records(gpu_inspect(16000, 10000, data), I.oracle_records(16000, 10000, data), "random, n_frames %d" % n)


def test_zero_frames_launches_nothing():
    torch = torch_mod()
    d_in = torch.zeros(150, dtype=torch.uint8, device="cuda")
    d_info = torch.full((1, I.WORDS), -7, dtype=torch.int32, device="cuda")
    pkg.inspect(10000, 48000, d_in, d_info, 150, 0)
    torch.cuda.synchronize()
    assert (d_info.cpu().numpy() == -7).all()


def test_ordered_behind_a_kernel_that_writes_the_input():
    """enqueued right behind the kernel that writes d_in, on the same stream, without synchronisation in between"""
    torch = torch_mod()
    n = 8192
    clean = I.clean_frames(48000, 10000, 150, 64, seed=9)
    data = np.tile(clean, (n // 64, 1))
    data[::7] = I.random_frames(len(data[::7]), 150, np.random.default_rng(9))
    ref = I.oracle_records(48000, 10000, data)
    key = 0x5A
    d_src = _dev(data ^ np.uint8(key))
    d_in = torch.zeros((n, 150), dtype=torch.uint8, device="cuda")
    d_info = torch.zeros((n, I.WORDS), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = torch.randn(2048, 2048, device="cuda")
        for _ in range(8):
            a = a @ a / 64.0  # keeps the stream busy before the writing kernel
        torch.bitwise_xor(d_src, key, out=d_in)
        pkg.inspect(10000, 48000, d_in, d_info, 150, n, stream=s.cuda_stream)
    s.synchronize()
    _assert_records(d_info.cpu().numpy(), ref, "stream order")


def test_in_a_process_without_any_codec_handle():
    """the call registers the configuration and fills the tables itself (a fresh process that never created an encoder or decoder)"""
    code = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import inspect_lib as I
pkg = importlib.import_module("lc3-codec_amd")
data = I.clean_frames(24000, 7500, 60, 100)
data[::3] = I.random_frames(len(data[::3]), 60, np.random.default_rng(1))
d_info = torch.zeros((100, 32), dtype=torch.int32, device="cuda")
pkg.inspect(7500, 24000, torch.from_numpy(data).cuda(), d_info, 60, 100)
torch.cuda.synchronize()
assert np.array_equal(d_info.cpu().numpy(), I.oracle_records(24000, 7500, data))
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_argument_errors():
    torch = torch_mod()
    L = pkg.load_library()
    d_in = torch.zeros(400, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros((1, I.WORDS), dtype=torch.int32, device="cuda")
    a, b = d_in.data_ptr(), d_info.data_ptr()
    assert L.lc3gpu_inspect(10000, 48000, None, None, None, 150, 1, b, None) == -1
    assert L.lc3gpu_inspect(10000, 48000, a, None, None, 150, 1, None, None) == -1
    assert L.lc3gpu_inspect(10000, 48000, a, None, None, 150, -1, b, None) == -1
    assert L.lc3gpu_inspect(10000, 48000, a, None, None, 0, 1, b, None) == -3
    assert L.lc3gpu_inspect(10000, 48000, a, None, None, 401, 1, b, None) == -3
    assert L.lc3gpu_inspect(5000, 48000, a, None, None, 150, 1, b, None) == -1
    assert L.lc3gpu_inspect(10000, 22050, a, None, None, 150, 1, b, None) == -1
    assert L.lc3gpu_inspect(10000, 48000, a, None, None, 150, 0, b, None) == 0
    with pytest.raises(pkg.Lc3GpuError):
        pkg.inspect(10000, 48000, d_in, d_info, 401, 1)
    assert L.lc3gpu_inspect(7500, 8000, a, None, None, 1, 1, b, None) == 0
    torch.cuda.synchronize()
    assert d_info.cpu().numpy()[0, 0] == I.SIDE_INFO + 1  # one byte: the side information cannot be read
