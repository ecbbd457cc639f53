"""lc3gpu-tool inspect -- the reference's examples/read_sideinfo.rs on the GPU: a WAV encoded by the tool, and a damaged copy of the .lc3
file, inspected frame by frame; every printed record equals the oracle's (lc3o_dec_side_info + lc3o_dec_arith) with its channel, frame
index and status name."""
import importlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import inspect_lib as I

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")
synth = importlib.import_module("lc3-codec_amd.synth")


@pytest.fixture(scope="module")
def tool():
    pkg.build_native()
    return pkg.build_tool()


def _wav_bytes(pcm_interleaved, fs, channels):
    data = pcm_interleaved.astype("<i2").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, channels, fs, fs * channels * 2,
                                                                                  channels * 2, 16)
    return hdr + b"data" + struct.pack("<I", len(data)) + data


def _expected(raw, fs, us, nbytes, channels):
    frames = np.frombuffer(raw[:len(raw) // nbytes * nbytes], np.uint8).reshape(-1, nbytes)
    recs = I.oracle_records(fs, us, frames)
    out = []
    for i, r in enumerate(recs):
        rec = np.zeros(1, api.FRAME_INFO_DTYPE)
        rec.view(np.int32)[:] = r
        d = {"channel": i % channels, "frame": i // channels}
        for name in api.FRAME_INFO_DTYPE.names:
            v = rec[name][0]
            d[name] = v.tolist() if isinstance(v, np.ndarray) else int(v)
        d["status"] = api.frame_status_name(r[0])
        out.append(d)
    return out


def _inspect(tool, path, fs, us, nbytes, channels):
    r = subprocess.run([tool, "inspect", str(path), str(fs), str(us), str(nbytes), str(channels)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.strip()]


@pytest.mark.parametrize("fs,us,channels,nbytes", [(48000, 10000, 2, 150), (16000, 7500, 1, 40)])
def test_inspect_encoded_and_damaged_files(tool, tmp_path, fs, us, channels, nbytes):
    nf = fs * us // 1000000
    n_frames = 60
    planar = synth.make_pcm(channels, n_frames, nf, fs)
    inter = planar.reshape(channels, n_frames * nf).T
    wav, lc3, broken = tmp_path / "in.wav", tmp_path / "out.lc3", tmp_path / "broken.lc3"
    wav.write_bytes(_wav_bytes(inter.reshape(-1), fs, channels))
    r = subprocess.run([tool, "encode", str(wav), str(lc3), str(fs), str(channels), str(us), str(nbytes)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    raw = lc3.read_bytes()
    assert len(raw) == n_frames * channels * nbytes
    got = _inspect(tool, lc3, fs, us, nbytes, channels)
    assert got == _expected(raw, fs, us, nbytes, channels)
    assert all(g["status"] == "Ok" for g in got)
    # a damaged copy: flipped bits and random runs in a third of the frames, and a trailing partial frame (not a frame)
    rng = np.random.default_rng(nbytes)
    frames = np.frombuffer(raw, np.uint8).reshape(-1, nbytes).copy()
    for i in range(0, len(frames), 3):
        k = int(rng.integers(0, nbytes))
        frames[i, k:k + 12] = rng.integers(0, 256, min(12, nbytes - k), dtype=np.uint8)
        frames[i, int(rng.integers(0, nbytes))] ^= np.uint8(1 << int(rng.integers(8)))
    damaged = frames.tobytes() + bytes(nbytes // 2)
    broken.write_bytes(damaged)
    got = _inspect(tool, broken, fs, us, nbytes, channels)
    want = _expected(damaged, fs, us, nbytes, channels)
    assert len(got) == n_frames * channels and got == want
    assert any(g["status"] != "Ok" for g in got)
