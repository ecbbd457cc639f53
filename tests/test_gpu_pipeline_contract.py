"""What include/lc3gpu.h promises of lc3gpu_pipeline beyond a plain round trip, on the GPU: a refused submission has launched nothing on
any group, the groups' slices may move between submissions, given group boundaries are taken as given, a mark stands behind an encode
queued alone.  48 kHz / 10 ms / 150 bytes, 8 channels -- two groups of four, the smallest pipeline that has a second group -- and 2
frames per submission unless a test says otherwise; every comparison exact, against the oracle and against plain handles on one stream.

These are outcome checks: kernels usually finish in submission order, so a missing wait would pass them almost every time.  That the
waits are queued is proved on the CPU, against a happens-before model of the runtime (tests/test_pipeline_hb.py)."""
import ctypes
import importlib

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")
synth = importlib.import_module("lc3-codec_amd.synth")
FS, US, NB, NF = pkg.SamplingFrequency.Hz48000, pkg.FrameDuration.TenMs, 150, 480
S, T_ALL = 8, 12
EPAIR, EINVAL = -8, -1


def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch


@pytest.fixture(scope="module")
def ref():
    """12 consecutive frames of 8 streams and what the oracle makes of them (computed once, never written)"""
    pcm = synth.make_pcm(S, T_ALL, NF, 48000, seed=71)
    ref_b = O.encode_batch(pcm, NB)
    ref_p = O.decode_batch(ref_b, NF)
    for a in (pcm, ref_b, ref_p):
        a.setflags(write=False)
    return pcm, ref_b, ref_p


def _pipeline():
    pl = pkg.Lc3Pipeline(S, US, FS)
    assert [(g["first"], g["n"]) for g in pl.groups] == [(0, 4), (4, 4)]
    return pl


def _dev(a):
    return torch_mod().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("group,role", [(1, "enc"), (0, "dec")])
def test_a_submission_refused_for_a_pair_flag_has_launched_nothing(ref, group, role):
    """the pair flag up on group 1's encoder (group 0 comes first in every loop) or on group 0's decoder (its own encoder comes first):
    lc3gpu_pipeline_submit returns LC3GPU_EPAIR, no group's state has moved, no byte is written, and the repeated submission is the
    oracle's for all 8 channels"""
    torch = torch_mod()
    pcm, ref_b, ref_p = ref
    pl = _pipeline()
    d_b = [torch.zeros((S, 2, NB), dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_o = [torch.zeros((S, 2, NF), dtype=torch.int16, device="cuda") for _ in range(2)]
    d_first = _dev(pcm[:, 0:2])  # (held until the pipeline is done with it: its streams are not the allocator's)
    pl.submit(d_first, d_b[0], d_o[0], NB, 2)
    pl.wait()
    assert np.array_equal(d_b[0].cpu().numpy(), ref_b[:, 0:2]) and np.array_equal(d_o[0].cpu().numpy(), ref_p[:, 0:2])
    handles = [g[r] for g in pl.groups for r in ("enc", "dec")]
    before = [h.state_save() for h in handles]
    flagged = pl.groups[group][role]
    assert not any(h.pair_pending() for h in handles)
    flagged.debug_pair_giveup()  # (the injection entry point: what a pair half that gives up does)
    assert [h.pair_pending() for h in handles] == [h is flagged for h in handles]
    d_in = _dev(pcm[:, 2:4])
    with pytest.raises(pkg.Lc3GpuError) as e:
        pl.submit(d_in, d_b[1], d_o[1], NB, 2)
    assert e.value.code == EPAIR
    torch.cuda.synchronize()
    after = [h.state_save() for h in handles]
    for h, a, b in zip(handles, before, after):
        assert np.array_equal(a, b), "a handle's state moved in a submission that was refused"
    assert not bool(d_b[1].any()) and not bool(d_o[1].any())
    assert not any(h.pair_pending() for h in handles)  # said once
    pl.submit(d_in, d_b[1], d_o[1], NB, 2)
    pl.wait()
    assert np.array_equal(d_b[1].cpu().numpy(), ref_b[:, 2:4]) and np.array_equal(d_o[1].cpu().numpy(), ref_p[:, 2:4])
    assert [h.pair_timeouts() for h in handles] == [int(h is flagged) for h in handles]
    # ... and the groups' state is that of plain handles that ran the same four frames on one stream
    enc, dec = pkg.Lc3Encoder(4, US, FS), pkg.Lc3Decoder(4, US, FS)
    d_b4 = torch.zeros((4, 2, NB), dtype=torch.uint8, device="cuda")
    d_o4 = torch.zeros((4, 2, NF), dtype=torch.int16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for t0 in (0, 2):
        enc.encode(_dev(pcm[4:8, t0:t0 + 2]), d_b4, NB, 2, stream=stream)
        dec.decode(d_b4, d_o4, NB, 2, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_b4.cpu().numpy(), ref_b[4:8, 2:4]) and np.array_equal(d_o4.cpu().numpy(), ref_p[4:8, 2:4])
    assert np.array_equal(pl.groups[1]["enc"].state_save(), enc.state_save()) and np.array_equal(pl.groups[1]["dec"].state_save(), dec.state_save())
    pl.close()


def test_n_frames_changing_between_submissions_into_one_byte_buffer(ref):
    """n_frames 4, 2, 4, 1 into ONE byte buffer and (a wait each, as the header asks for an output buffer whose slices move) one output
    buffer: group 1's slice starts where group 0's of another n_frames lies; every step the oracle's"""
    torch = torch_mod()
    pcm, ref_b, ref_p = ref
    pl = _pipeline()
    d_b = torch.zeros(S * 4 * NB, dtype=torch.uint8, device="cuda")
    d_o = torch.zeros(S * 4 * NF, dtype=torch.int16, device="cuda")
    t0 = 0
    for n in (4, 2, 4, 1):
        d_in = _dev(pcm[:, t0:t0 + n])
        pl.submit(d_in, d_b, d_o, NB, n)
        pl.wait()
        got_b = d_b.cpu().numpy()[:S * n * NB].reshape(S, n, NB)
        got_p = d_o.cpu().numpy()[:S * n * NF].reshape(S, n, NF)
        assert np.array_equal(got_b, ref_b[:, t0:t0 + n]) and np.array_equal(got_p, ref_p[:, t0:t0 + n]), (t0, n)
        t0 += n
    for g in pl.groups:
        assert g["enc"].pair_timeouts() == 0 and g["dec"].pair_timeouts() == 0
    pl.close()


def test_a_mixed_pipeline_with_given_boundaries_and_the_boundaries_it_refuses():
    """four streams of two configurations, group_first = [0, 2] (a stream of either configuration in either group): one round trip is the
    per-configuration oracle's; boundaries given with a group count of 0 or of more than n_streams are LC3GPU_EINVAL (the count is the
    length of the caller's array: a default or a clamp would read past it or reinterpret it)"""
    torch = torch_mod()
    cfgs = [(48000, 10000, 150), (32000, 7500, 80)]
    descs = [cfgs[0], cfgs[1], cfgs[0], cfgs[1]]
    T = 2
    streams = []
    for i, (fs, us, nb) in enumerate(descs):
        nf = pkg.Lc3Config(fs, us).nf
        x = synth.make_pcm(1, T, nf, fs, seed=90 + i)
        b = O.encode_batch(x, nb, fs_hz=fs, frame_us=us)
        streams.append((x, b, O.decode_batch(b, nf, fs_hz=fs, frame_us=us)))
    pl = pkg.Lc3Pipeline.mixed(descs, group_first=[0, 2])
    assert [(g["first"], g["n"]) for g in pl.groups] == [(0, 2), (2, 2)]
    d_pcm = _dev(np.concatenate([x.reshape(-1) for x, _, _ in streams]))
    d_b = torch.zeros(sum(b.size for _, b, _ in streams), dtype=torch.uint8, device="cuda")
    d_o = torch.zeros(sum(p.size for _, _, p in streams), dtype=torch.int16, device="cuda")
    pl.submit_mixed(d_pcm, d_b, d_o, T)
    pl.wait()
    assert np.array_equal(d_b.cpu().numpy(), np.concatenate([b.reshape(-1) for _, b, _ in streams]))
    assert np.array_equal(d_o.cpu().numpy(), np.concatenate([p.reshape(-1) for _, _, p in streams]))
    pl.close()
    L = pkg.load_library()
    for n_groups, gf in ((0, [0]), (0, [0, 2]), (5, [0, 1, 2, 3, 4])):
        h = ctypes.c_void_p()
        rc = L.lc3gpu_pipeline_create_mixed(ctypes.byref(h), len(descs), api._desc_array(descs), n_groups, (ctypes.c_int * len(gf))(*gf))
        assert rc == EINVAL and not h.value, (n_groups, gf)
    for n_groups in (0, 5):  # without boundaries the count is a wish, as before: the default, or as many groups as there are streams
        p2 = pkg.Lc3Pipeline.mixed(descs, n_groups=n_groups)
        assert len(p2.groups) == (2 if n_groups == 0 else 4)
        p2.close()


def test_a_mark_after_an_encode_queued_alone_stands_behind_it(ref):
    """submit, then lc3gpu_pipeline_encode, then a mark: once the mark's event has completed the encode's bytes are the oracle's (the
    last group's latest work is then on its encoder stream, not on the decoder stream it has also used)"""
    torch = torch_mod()
    pcm, ref_b, ref_p = ref
    pl = _pipeline()
    d_b = [torch.zeros((S, 2, NB), dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_o = torch.zeros((S, 2, NF), dtype=torch.int16, device="cuda")
    d_in = [_dev(pcm[:, 0:2]), _dev(pcm[:, 2:4])]
    ev = torch.cuda.Event()
    ev.record()  # (gives the event its handle)
    torch.cuda.synchronize()
    pl.submit(d_in[0], d_b[0], d_o, NB, 2)
    pl.encode(d_in[1], d_b[1], NB, 2)
    pl.mark(ev)
    ev.synchronize()
    last = pl.groups[-1]
    got = d_b[1][last["first"]:last["first"] + last["n"]].cpu().numpy()  # (the mark speaks for the last group only)
    assert np.array_equal(got, ref_b[last["first"]:, 2:4])
    pl.wait()
    assert np.array_equal(d_b[1].cpu().numpy(), ref_b[:, 2:4]) and np.array_equal(d_o.cpu().numpy(), ref_p[:, 0:2])
    pl.close()


def test_a_submission_refused_for_its_arguments_has_launched_nothing(ref):
    """d_pcm_out only 2-byte aligned is what group 0's DECODER would refuse, after group 0's encoder has launched: the pipeline refuses it
    first (LC3GPU_EINVAL), no group's state has moved, no byte is written, and the corrected submission is the oracle's"""
    torch = torch_mod()
    pcm, ref_b, ref_p = ref
    pl = _pipeline()
    handles = [g[r] for g in pl.groups for r in ("enc", "dec")]
    d_in = _dev(pcm[:, 0:2])
    d_b = torch.zeros((S, 2, NB), dtype=torch.uint8, device="cuda")
    d_o = torch.zeros(S * 2 * NF + 2, dtype=torch.int16, device="cuda")
    before = [h.state_save() for h in handles]
    for kind, args in (("submit", (d_in, d_b, d_o[1:], NB, 2)), ("submit", (d_in.reshape(-1)[1:], d_b, d_o, NB, 2)), ("submit", (d_in, d_b, d_o, 19, 2)),
                       ("decode", (d_b, d_o[1:], NB, 2)), ("encode", (d_in, d_b, 401, 2))):
        with pytest.raises(pkg.Lc3GpuError) as e:
            getattr(pl, kind)(*args)
        assert e.value.code == (EINVAL if args[-2] == NB else -3), (kind, args[-2])  # (-3: LC3GPU_ELENGTH)
    torch.cuda.synchronize()
    for a, b in zip(before, [h.state_save() for h in handles]):
        assert np.array_equal(a, b), "a handle's state moved in a submission that was refused"
    assert not bool(d_b.any()) and not bool(d_o.any())
    pl.submit(d_in, d_b, d_o, NB, 2)
    pl.wait()
    assert np.array_equal(d_b.cpu().numpy(), ref_b[:, 0:2]) and np.array_equal(d_o.cpu().numpy()[:S * 2 * NF].reshape(S, 2, NF), ref_p[:, 0:2])
    pl.close()


def test_a_decode_alone_takes_the_frame_sizes_a_decoder_takes(ref):
    """a decoder handle takes 1..400 bytes per frame, an encoder 20..400: lc3gpu_pipeline_decode of 10-byte frames is the oracle's on fresh
    channels, and between two ordinary decodes it is what a plain decoder handle makes of the same three calls on one stream"""
    torch = torch_mod()
    pcm, ref_b, ref_p = ref
    b10 = np.random.default_rng(5).integers(0, 256, (S, 2, 10), dtype=np.uint8)
    pl = _pipeline()
    dec = pkg.Lc3Decoder(S, US, FS)
    stream = torch.cuda.current_stream().cuda_stream
    d_b10, d_b150 = _dev(b10), _dev(ref_b[:, 0:2])
    outs_pl = [torch.zeros((S, 2, NF), dtype=torch.int16, device="cuda") for _ in range(4)]
    outs_h = [torch.zeros((S, 2, NF), dtype=torch.int16, device="cuda") for _ in range(4)]
    for k, (d_b, nb) in enumerate(((d_b10, 10), (d_b150, NB), (d_b10, 10), (d_b150, NB))):
        pl.decode(d_b, outs_pl[k], nb, 2)
        dec.decode(d_b, outs_h[k], nb, 2, stream=stream)
    pl.wait()
    torch.cuda.synchronize()
    assert np.array_equal(outs_pl[0].cpu().numpy(), O.decode_batch(b10, NF))
    for k in range(4):
        assert np.array_equal(outs_pl[k].cpu().numpy(), outs_h[k].cpu().numpy()), k
    pl.close()
