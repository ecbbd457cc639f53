"""The composed corpus on the GPU (composed_corpus.py: frames with chosen contents in the corners of the LC3 format that the project's own
encoder never writes, census_lib.cells() names them): lc3gpu_decode at all 12 configurations in the full-batch form and once more per
kernel form in fresh child processes, lc3gpu_decode_vbr over the size-dependent cells with a size per frame, lc3gpu_inspect on every
composed frame, and one lc3gpu_decode_mixed_views tick with the streams of all configurations in one handle.  The oracle is the
yardstick; identical 16-bit PCM and identical records, no tolerance."""
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import composed_corpus as CC
import inspect_lib as I
import test_gpu_inspect as GI
import test_gpu_mixed_list as ML

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("lc3-codec_amd")
ROOT = ML.ROOT
torch_mod = ML.torch_mod
FORMS = [{"LC3GPU_RECON": "lane"}, {"LC3GPU_RECON": "late"}, {"LC3GPU_RECON": "wave"}, {"LC3GPU_PARSE_PC": "0"}, {"LC3GPU_FPB": "64"}, {"LC3GPU_FPB": "256"}]


def decode_tiled(fs, us, nbytes, data, ref, more_than):
    """lc3gpu_decode over data uint8[S0][T][nbytes], repeated over so many streams that the call holds more than `more_than` frames (the
    default dispatch then takes the full-batch producer / consumer parser); every copy against ref int16[S0][T][nf], on the device.
    -> (stream, frame) pairs of the first copy that differs, largest difference"""
    torch = torch_mod()
    S0, T, _ = data.shape
    reps = more_than // (S0 * T) + 1
    nf = ref.shape[2]
    d_in = torch.from_numpy(np.ascontiguousarray(data)).cuda().repeat(reps, 1, 1)
    d_pcm = torch.full((reps * S0, T, nf), 12345, dtype=torch.int16, device="cuda")
    dec = pkg.Lc3Decoder(reps * S0, us, fs)
    dec.decode(d_in, d_pcm, nbytes, T, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert dec.pair_timeouts() == 0
    dec.close()
    want = torch.from_numpy(np.ascontiguousarray(ref)).cuda()
    bad = (d_pcm.view(reps, S0, T, nf) != want[None]).any(3)
    if not bool(bad.any()):
        return [], 0
    r = int(bad.any(2).any(1).nonzero()[0])
    got = d_pcm.view(reps, S0, T, nf)[r].cpu().numpy()
    return [tuple(v) for v in np.argwhere((got != ref).any(2))], int(np.abs(got.astype(np.int64) - ref).max())


def check_decode(fs, us, groups, refs, more_than, what=""):
    for nbytes, (names, data) in groups.items():
        bad, worst = decode_tiled(fs, us, nbytes, data, refs[nbytes], more_than)
        assert not bad, "%d Hz / %d us, %d bytes%s: %d frames differ from the oracle, largest difference %d; first: stream %s frame %d" % (
            fs, us, nbytes, what, len(bad), worst, names[bad[0][0]], bad[0][1])


@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_decode_composed_against_the_oracle(fs, us):
    check_decode(fs, us, CC.by_size(fs, us), CC.oracle_pcm(fs, us), ML._pc_threshold())


_FORMS_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_composed as m
z = np.load(sys.argv[2])
for fs, us in m.I.CONFIGS:
    sizes = [int(k.split("_")[3]) for k in z.files if k.startswith("data_%d_%d_" % (fs, us))]
    groups = {n: (z["names_%d_%d_%d" % (fs, us, n)].tolist(), z["data_%d_%d_%d" % (fs, us, n)]) for n in sizes}
    refs = {n: z["pcm_%d_%d_%d" % (fs, us, n)] for n in sizes}
    m.check_decode(fs, us, groups, refs, int(sys.argv[3]), " under %s" % sys.argv[4])
print("forms ok")
"""


def test_decode_composed_every_kernel_form_in_a_fresh_process():
    """the same decode parity under LC3GPU_RECON = lane, late and wave, LC3GPU_PARSE_PC = 0 and LC3GPU_FPB = 64 and 256: one child per form
    (the forms are read once per process), each under its own time limit; stops at the first child that fails.  The children load the
    corpus and the oracle's PCM from a file this process writes"""
    arrays = {}
    for fs, us in I.CONFIGS:
        refs = CC.oracle_pcm(fs, us)
        for n, (names, data) in CC.by_size(fs, us).items():
            arrays["names_%d_%d_%d" % (fs, us, n)] = np.array(names)
            arrays["data_%d_%d_%d" % (fs, us, n)] = data
            arrays["pcm_%d_%d_%d" % (fs, us, n)] = refs[n]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "composed.npz")
        np.savez(path, **arrays)
        for env in FORMS:
            e = dict(os.environ)
            e.update(env)
            r = subprocess.run([sys.executable, "-c", _FORMS_CHILD, ROOT, path, str(ML._pc_threshold()), str(env)], env=e, capture_output=True, text=True,
                               timeout=600)
            assert r.returncode == 0 and "forms ok" in r.stdout, (env, r.returncode, r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_decode_vbr_sizes_changing_within_a_stream(fs, us):
    """the cells that hang on the frame size (filter gain, rate_flag, lpc_weighting, lsb_mode) in one lc3gpu_decode_vbr launch in which every
    stream changes its size from frame to frame"""
    torch = torch_mod()
    names, data, nb = CC.sized_streams(fs, us)
    assert all(len(set(row.tolist())) >= 3 for row in nb)
    ref = CC.oracle_pcm_sized(fs, us)
    dec = pkg.Lc3Decoder(len(data), us, fs)
    d_pcm = torch.full(ref.shape, 12345, dtype=torch.int16, device="cuda")
    dec.decode_vbr(torch.from_numpy(data).cuda(), torch.from_numpy(nb.view(np.int16)).cuda(), d_pcm, 400, CC.T, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_pcm.cpu().numpy()
    bad = np.argwhere((got != ref).any(2))
    assert len(bad) == 0, "%d Hz / %d us: %d frames differ from the oracle, largest difference %d; first: stream %d frame %d (%d bytes, from %s)" % (
        fs, us, len(bad), np.abs(got.astype(np.int64) - ref).max(), bad[0][0], bad[0][1], nb[tuple(bad[0])], names[(bad[0][0] + bad[0][1]) % len(names)])
    assert dec.plc_events() == 0  # the reject cells hang on no size: none among these streams


@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_inspect_composed_against_the_oracle(fs, us):
    """every composed frame's record, the reject cells included, and status != 0 exactly where the decoder conceals"""
    streams = CC.corpus(fs, us)
    frames = [f for _, fr in streams for f in fr]
    data = np.zeros((len(frames), 400), np.uint8)
    for i, f in enumerate(frames):
        data[i, :len(f)] = f
    nb = np.array([len(f) for f in frames], np.uint16)
    ref = I.oracle_records(fs, us, data, nb)
    got = GI.gpu_inspect(fs, us, data, nb)
    GI._assert_records(got, ref, "%d Hz / %d us, composed" % (fs, us))
    lost = got[:, 0] != 0
    assert lost.sum() >= 8, "the reject cells"
    assert np.array_equal(lost, I.oracle_plc(fs, us, data, nb, streams=len(streams)))
    assert GI._decode_plc(fs, us, data, None, len(streams), nb) == lost.sum()


def test_mixed_views_tick_with_all_configurations():
    """one lc3gpu_decode_mixed_views call that carries every composed stream of all 12 configurations, each a channel of one mixed handle
    and a view with the stream's own frame size, frames and PCM back to back"""
    torch = torch_mod()
    descs, views, blobs, want = [], [], [], []
    pcm_off = byte_off = 0
    for fs, us in I.CONFIGS:
        refs = CC.oracle_pcm(fs, us)
        for n, (names, data) in CC.by_size(fs, us).items():
            for s in range(len(names)):
                views.append(dict(channel=len(descs), n_frames=CC.T, nbytes=n, pcm_off=pcm_off, byte_off=byte_off))
                descs.append((fs, us, CC.base_size(fs, us)))  # one group per configuration; the view names the stream's own size
                blobs.append(data[s].reshape(-1))
                want.append(refs[n][s].reshape(-1))
                pcm_off, byte_off = pcm_off + want[-1].size, byte_off + blobs[-1].size
    order = np.random.default_rng(12).permutation(len(views))  # the views in any order, as a tick has them
    want = np.concatenate(want)
    dec = pkg.Lc3Decoder.mixed(descs)
    d_pcm = torch.full((want.size,), 12345, dtype=torch.int16, device="cuda")
    dec.decode_mixed_views([views[i] for i in order], torch.from_numpy(np.concatenate(blobs)).cuda(), d_pcm, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_pcm.cpu().numpy()
    bad = [i for i, v in enumerate(views) if not np.array_equal(got[v["pcm_off"]:v["pcm_off"] + CC.T * dec.configs[i].nf], want[v["pcm_off"]:v["pcm_off"] + CC.T * dec.configs[i].nf])]
    assert not bad, "%d of %d views differ from the oracle; first: channel %d %s at %d bytes" % (len(bad), len(views), bad[0], descs[bad[0]][:2], views[bad[0]]["nbytes"])
    assert np.array_equal(got, want) and dec.pair_timeouts() == 0


@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_encode_and_decode_corner_pcm_against_the_oracle(fs, us):
    """the encoder's corner PCM (corner_pcm.py) at 20, 80 and 400 bytes: lc3gpu_encode byte-exact against the oracle encoder (8 kHz under
    LC3GPU_SPEC_8KHZ_ENCODE), then lc3gpu_decode of those frames against the oracle's PCM"""
    import corner_pcm as P
    import oracle_lib as O
    import test_corner_pcm as TP

    torch = torch_mod()
    st = torch.cuda.current_stream().cuda_stream
    flags = 1 if fs == 8000 else 0
    nf = I.config(fs, us).nf
    for kind in P.KINDS:
        for nbytes in TP.SIZES:
            pcm, ref = TP.oracle_bytes(kind, fs, us, nbytes)
            S = len(pcm)
            enc = pkg.Lc3Encoder(S, us, fs, spec_flags=flags)
            d_out = torch.full((S, TP.T, nbytes), 0xA5, dtype=torch.uint8, device="cuda")
            enc.encode(torch.from_numpy(pcm).cuda(), d_out, nbytes, TP.T, stream=st)
            torch.cuda.synchronize()
            bad = np.argwhere((d_out.cpu().numpy() != ref).any(2))
            assert len(bad) == 0, "%s at %d Hz / %d us / %d bytes: frames (stream, frame) differing from the oracle encoder: %s" % (kind, fs, us, nbytes, bad[:8].tolist())
            dec = pkg.Lc3Decoder(S, us, fs)
            d_pcm = torch.full((S, TP.T, nf), 12345, dtype=torch.int16, device="cuda")
            dec.decode(d_out, d_pcm, nbytes, TP.T, stream=st)
            torch.cuda.synchronize()
            assert np.array_equal(d_pcm.cpu().numpy(), O.decode_batch(ref, nf, fs, us)), "%s at %d Hz / %d us / %d bytes: decoded PCM" % (kind, fs, us, nbytes)
            enc.close()
            dec.close()
