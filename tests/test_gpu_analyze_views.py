"""lc3gpu_analyze_mixed_views on the GPU: the reconstructed spectrum, the 64 band energies and the total energy of every frame of a tick,
read where the frames lie (ring slots behind packet headers) and written at the frames' flag indices.  Yardsticks: the oracle's stage chain
and the two energy formulas evaluated sequentially in float32 (analyze_views_lib), lc3gpu_inspect_mixed_views on the same arguments, and
the LC3GPU_DBG_SPEC dump of lc3gpu_decode_frame_debug.  After every call the WHOLE output arrays are compared bit for bit, sentinels
between and around the frames included."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import analyze_views_lib as A
import inspect_lib as I
from inspect_views_lib import view, views_of

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ECHANNEL, ELENGTH = 0, -1, -2, -3
SIZES = (1, 6, 7, 20, 40, 150, 400)


def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch


def dev(a):
    return torch_mod().from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared fixtures are read-only)


def cur_stream():
    return torch_mod().cuda.current_stream().cuda_stream


def fresh_outputs(n_out):
    torch = torch_mod()
    s = float(A.SENTINEL)
    return (torch.full((n_out,), s, dtype=torch.float32, device="cuda"), torch.full((n_out, A.BANDS), s, dtype=torch.float32, device="cuda"),
            torch.full((n_out, A.LINES), s, dtype=torch.float32, device="cuda"))


def run(an, vs, d_in, d_flags, n_out, want="ebs", stream=None):
    """one call on fresh sentinel-filled outputs -> (energy, bands, spec) as numpy"""
    e, b, s = fresh_outputs(n_out)
    an.analyze_mixed_views(vs, d_in, e if "e" in want else None, b if "b" in want else None, s if "s" in want else None, d_bad_frame=d_flags,
                           stream=cur_stream() if stream is None else stream)
    torch_mod().cuda.synchronize()
    return e.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy()


def assert_outputs(got, want, what):
    for name, g, w in zip(("energies", "band rows", "spectrum rows"), got, want):
        g2, w2 = g.reshape(len(g), -1).view(np.uint32), w.reshape(len(w), -1).view(np.uint32)
        bad = np.nonzero((g2 != w2).any(1))[0]
        assert not len(bad), "%s: %d %s differ; first at %d\nexpected %s\ngpu      %s" % (what, len(bad), name, bad[0], w.reshape(len(w), -1)[bad[0]][:8],
                                                                                         g.reshape(len(g), -1)[bad[0]][:8])


def _frames_of_size(fs, us, size, n, rng):
    """n frames of `size` bytes of one configuration, about 4 % of them damaged or flagged: clean frames from the oracle encoder where the
    size carries a frame (20 bytes and up), random bytes below"""
    if size >= 20:
        fr = np.array(I.clean_frames(fs, us, size, n, seed=size + n), np.uint8)
    else:
        fr = I.random_frames(n, size, rng)
    hit = rng.random(n) < 0.03
    if hit.any():
        fr[hit] = I.damage(fr[hit], rng)[0]
    return [(bytes(fr[t]), int(rng.random() < 0.015)) for t in range(n)]


@pytest.fixture(scope="module")
def the_tick():
    """all 12 configurations in one call, sizes 1 .. 400 (so that a workgroup has 64 lanes), rings of 8 slots of 400 bytes behind 12-byte
    headers; three (configuration, size) buckets hold 63, 64 and 65 frames.  With what the call must leave (computed once, never written)"""
    rng = np.random.default_rng(4242)
    assert api.analyzer_plan_info(400)[0] == 64
    descs = [(fs, us, 40) for fs, us in I.CONFIGS]
    items = []
    counts = {(0, 20): 63, (5, 40): 64, (11, 150): 65}
    for ch, (fs, us) in enumerate(I.CONFIGS):
        for size in SIZES:
            n = counts.get((ch, size), int(rng.integers(3, 12)))
            frames = _frames_of_size(fs, us, size, n, rng)
            for k in range(0, n, 8):
                items.append((ch, size, frames[k: k + 8]))
    vs, d_in, flags, n_out, placed = A.ring_tick(items, rng=rng)
    want = A.expected_outputs(placed, descs, n_out)
    for a in (vs, d_in, flags) + want:
        a.setflags(write=False)
    return descs, vs, d_in, flags, n_out, placed, want


@pytest.fixture(scope="module")
def the_other_input(the_tick):
    """the tick with every byte complemented -- other spectra, other verdicts, the same places -- and what a call over it must leave"""
    descs, vs, d_in, flags, n_out, placed, want = the_tick
    alt_in = (~np.asarray(d_in)).astype(np.uint8)
    alt_want = A.expected_outputs([(i, ch, bytes((~np.frombuffer(fr, np.uint8)).astype(np.uint8)), fl) for i, ch, fr, fl in placed], descs, n_out)
    assert not A.same_bits(alt_want[0], want[0])
    for a in (alt_in,) + alt_want:
        a.setflags(write=False)
    return alt_in, alt_want


def test_the_tick_in_rings_over_all_twelve_configurations(the_tick):
    descs, vs, d_in, flags, n_out, placed, want = the_tick
    at = np.array([p[0] for p in placed])
    lost = want[0][at] < 0
    big = np.array([len(p[2]) >= 20 for p in placed])  # (below 20 bytes the frames are random bytes: nearly all of them are refused)
    assert len(placed) > 600 and 0.01 < lost[big].mean() < 0.12 and lost[~big].any() and len(vs) > len(placed) // 8
    an = pkg.Lc3Analyzer(descs, len(vs), len(placed))
    assert_outputs(run(an, vs, dev(d_in), dev(flags), n_out), want, "the tick")
    an.close()


@pytest.mark.parametrize("size,fpb", [(40, 256), (150, 128), (400, 64)])
def test_frame_counts_around_each_of_the_three_workgroup_sizes(size, fpb):
    """buckets of fpb - 1, fpb and fpb + 1 frames in one call whose largest frame size gives fpb lanes per workgroup"""
    assert api.analyzer_plan_info(size)[0] == fpb
    rng = np.random.default_rng(size)
    cfgs = [(16000, 10000), (48000, 7500), (8000, 7500)]
    descs = [(fs, us, size) for fs, us in cfgs]
    items = []
    for ch, ((fs, us), n) in enumerate(zip(cfgs, (fpb - 1, fpb, fpb + 1))):
        frames = _frames_of_size(fs, us, size, n, rng)
        items += [(ch, size, frames[k: k + 8]) for k in range(0, n, 8)]
    vs, d_in, flags, n_out, placed = A.ring_tick(items, rng=rng)
    an = pkg.Lc3Analyzer(descs, len(vs), 3 * fpb)
    assert_outputs(run(an, vs, dev(d_in), dev(flags), n_out), A.expected_outputs(placed, descs, n_out), "%d lanes" % fpb)
    an.close()


def test_each_of_the_seven_output_forms_gives_the_same_values(the_tick):
    descs, vs, d_in, flags, n_out, placed, want = the_tick
    an = pkg.Lc3Analyzer(descs, len(vs), len(placed))
    d, f = dev(d_in), dev(flags)
    blank = [np.full_like(w, A.SENTINEL) for w in want]
    for form in ("e", "b", "s", "eb", "es", "bs", "ebs"):
        got = run(an, vs, d, f, n_out, form)
        assert_outputs(got, [w if c in form else z for c, w, z in zip("ebs", want, blank)], "outputs " + form)
    # without flags: every frame on its own bytes
    assert_outputs(run(an, vs, d, None, n_out), A.expected_outputs(placed, descs, n_out, use_flags=False), "no flags")
    # a band array that is only 4-byte aligned
    torch = torch_mod()
    raw = torch.full((n_out * A.BANDS + 1,), float(A.SENTINEL), dtype=torch.float32, device="cuda")
    an.analyze_mixed_views(vs, d, None, raw[1:], None, d_bad_frame=f, stream=cur_stream())
    torch.cuda.synchronize()
    assert raw.data_ptr() % 16 == 0 and raw[0].item() == float(A.SENTINEL)
    assert A.same_bits(raw[1:].cpu().numpy().reshape(n_out, A.BANDS), want[1])
    an.close()


def test_energy_is_negative_exactly_where_the_inspector_reports_a_status(the_tick):
    descs, vs, d_in, flags, n_out, placed, want = the_tick
    torch = torch_mod()
    d, f = dev(d_in), dev(flags)
    an = pkg.Lc3Analyzer(descs, len(vs), len(placed))
    insp = pkg.Lc3Inspector(descs, len(vs))
    e = run(an, vs, d, f, n_out, "e")[0]
    d_status = torch.full((n_out,), 0xCC, dtype=torch.uint8, device="cuda")
    insp.inspect_mixed_views(vs, d, d_status, None, d_bad_frame=f, stream=cur_stream())
    torch.cuda.synchronize()
    status = d_status.cpu().numpy()
    at = np.array([p[0] for p in placed])
    assert np.array_equal(e[at] < 0, status[at] != 0) and 0 < (status[at] != 0).sum() < len(at)
    assert (e[at][status[at] != 0] == -1.0).all()
    an.close()
    insp.close()


@pytest.mark.parametrize("fs,us,size", [(48000, 10000, 150), (24000, 7500, 60)])
def test_the_spectrum_is_the_debug_dump_of_the_decoder(fs, us, size):
    fr = np.array(I.clean_frames(fs, us, size, 6, seed=11), np.uint8)
    ne = I.config(fs, us).ne
    an = pkg.Lc3Analyzer([(fs, us, size)], 1, 6)
    d_spec = torch_mod().zeros((6, A.LINES), dtype=torch_mod().float32, device="cuda")
    an.analyze_mixed_views(views_of(view(n_frames=6)), dev(fr.reshape(-1)), None, None, d_spec, stream=cur_stream())
    torch_mod().cuda.synchronize()
    spec = d_spec.cpu().numpy()
    for t in range(6):
        dec = pkg.Lc3Decoder(1, us, fs)  # (fresh: the dump of a good frame does not depend on the frames before it, the decoder's state does)
        _, dbg = dec.decode_frame_debug(fr[t], recon_form=0)
        dec.close()
        assert A.same_bits(spec[t, :ne], dbg[api.DBG_SPEC: api.DBG_SPEC + ne]) and not spec[t, ne:].any(), (fs, us, t)
    an.close()


def test_a_ring_that_wraps_is_two_views_of_one_channel():
    rng = np.random.default_rng(8)
    fs, us, nb, SLOTS = 32000, 10000, 80, 8
    fr = np.array(I.clean_frames(fs, us, nb, 5, seed=3), np.uint8)
    fr[2] = I.random_frames(1, nb, rng)[0]
    ring = np.full(12 + SLOTS * 412, 0xEE, np.uint8)
    order = [6, 7, 0, 1, 2]  # the tick's five frames: the ring's last two slots, then its first three
    for t, s in enumerate(order):
        ring[12 + 412 * s: 12 + 412 * s + nb] = fr[t]
    vs = views_of(view(channel=0, n_frames=2, byte_off=12 + 412 * 6, byte_pitch=412, flag_off=6), view(channel=0, n_frames=3, byte_off=12, byte_pitch=412, flag_off=0))
    flags = np.zeros(SLOTS, np.uint8)
    flags[7] = 1
    placed = [(s, 0, bytes(fr[t]), int(flags[s])) for t, s in enumerate(order)]
    an = pkg.Lc3Analyzer([(fs, us, nb)], 2, 5)
    assert_outputs(run(an, vs, dev(ring), dev(flags), SLOTS), A.expected_outputs(placed, [(fs, us, nb)], SLOTS), "ring wrap")
    an.close()


def test_every_refusal_on_a_live_analyzer_leaves_the_outputs_alone(the_tick):
    descs, vs, d_in_h, flags_h, n_out, placed, want = the_tick
    torch = torch_mod()
    L = pkg.load_library()
    an = pkg.Lc3Analyzer(descs, len(vs), len(placed))
    d_in, d_flags = dev(d_in_h), dev(flags_h)
    d_e, d_b, d_s = fresh_outputs(n_out)
    one = view(channel=3, n_frames=4, byte_off=12, byte_pitch=412, flag_off=5, flag_pitch=2)
    P = lambda a: a.ctypes.data_as(api.ctypes.c_void_p)

    def call(v, n=None, h=an._h, din=d_in.data_ptr(), in_bytes=d_in.numel(), fl=d_flags.data_ptr(), n_flags=n_out, e=d_e.data_ptr(), n_e=n_out,
             b=d_b.data_ptr(), n_b=n_out, s=d_s.data_ptr(), n_s=n_out):
        return L.lc3gpu_analyze_mixed_views(h, None if v is None else P(v), len(v) if n is None else n, din, in_bytes, fl, n_flags, e, n_e, b, n_b, s, n_s,
                                            cur_stream())

    nb3 = 40
    v3 = views_of(view(n_frames=3, flag_off=7, flag_pitch=5))
    refused = [
        (call(views_of(view(channel=-1))), ECHANNEL), (call(views_of(view(channel=12))), ECHANNEL),
        (call(views_of(view(n_frames=0))), ELENGTH), (call(views_of(view(nbytes=401))), ELENGTH), (call(views_of(view(nbytes=-1))), ELENGTH),
        (call(views_of(view(n_frames=2**31 - 1, nbytes=1), view(n_frames=1, nbytes=1))), ELENGTH),
        (call(views_of(*([one] * (len(vs) + 1)))), ELENGTH),
        (call(views_of(view(n_frames=len(placed) + 1, nbytes=1))), ELENGTH),  # one frame more than max_frames
        (call(views_of(view(n_frames=3, byte_off=d_in.numel() - 2 * 412 - nb3 + 1, byte_pitch=412))), ELENGTH),
        (call(v3, n_flags=17), ELENGTH), (call(v3, n_e=17), ELENGTH), (call(v3, n_b=17), ELENGTH), (call(v3, n_s=17), ELENGTH),
        (call(views_of(view(byte_off=-1))), EINVAL), (call(views_of(view(flag_off=-1))), EINVAL),
        (call(views_of(view(n_frames=2, byte_pitch=nb3 - 1))), EINVAL), (call(views_of(view(n_frames=2, flag_pitch=-1))), EINVAL),
        (call(views_of(view(reserved=(0, 0, 1)))), EINVAL),
        (call(views_of(one), e=None, b=None, s=None), EINVAL), (call(views_of(one), h=None), EINVAL), (call(None, n=1), EINVAL),
        (call(views_of(one), din=None), EINVAL), (call(views_of(one), n=-1), EINVAL),
        (call(views_of(one), e=d_e.data_ptr() + 2), EINVAL), (call(views_of(one), b=d_b.data_ptr() + 1), EINVAL),
        (call(views_of(one), s=d_s.data_ptr() + 4), EINVAL), (call(views_of(one), s=d_s.data_ptr() + 8), EINVAL),
        (call(views_of(one), e=d_in.data_ptr() + 100), EINVAL), (call(views_of(one), e=d_flags.data_ptr(), n_e=4), EINVAL),
        (call(views_of(one), e=d_b.data_ptr() + 256, n_e=64), EINVAL), (call(views_of(one), b=d_s.data_ptr(), n_b=16), EINVAL),
        (call(views_of(one), s=d_in.data_ptr(), n_s=1), EINVAL), (call(views_of(one), b=d_flags.data_ptr(), n_b=1), EINVAL),
        (call(views_of(one), s=d_e.data_ptr(), n_s=16), EINVAL),
    ]
    torch.cuda.synchronize()
    for k, (rc, code) in enumerate(refused):
        assert rc == code, (k, rc, code)
    s32 = np.array([A.SENTINEL], np.float32).view(np.uint32)[0]
    for t in (d_e, d_b, d_s):
        assert (t.cpu().numpy().view(np.uint32) == s32).all()
    # accepted right at the ends (max_frames exactly), and no views at all
    assert call(views_of(view(n_frames=3, byte_off=d_in.numel() - 2 * 412 - nb3, byte_pitch=412, flag_off=n_out - 11, flag_pitch=5))) == OK
    assert call(views_of(view(n_frames=len(placed), nbytes=1, flag_pitch=0)), n_e=len(placed), b=None, s=None, fl=None) == OK
    assert call(vs[:0]) == OK
    torch.cuda.synchronize()
    assert (d_b.cpu().numpy().view(np.uint32) != s32).any(1).sum() == 3 and (d_s.cpu().numpy().view(np.uint32) != s32).any(1).sum() == 3
    # the analyzer still works
    assert_outputs(run(an, vs, d_in, d_flags, n_out), want, "after the refusals")
    an.close()


def test_forty_calls_queued_back_to_back_with_alternating_input(the_tick, the_other_input):
    """more calls in flight than the upload ring has slots, behind a kernel that keeps the stream busy, all through ONE analyzer's scratch
    columns: even calls read the tick, odd calls the tick with every byte complemented;
    every call's results are its own"""
    alt_in, alt_want = the_other_input
    descs, vs, d_in_h, flags_h, n_out, placed, want = the_tick
    torch = torch_mod()
    slots = api.analyzer_plan_info(400)[2]
    assert slots < 40
    an = pkg.Lc3Analyzer(descs, len(vs), len(placed))
    d_ins, d_flags = (dev(d_in_h), dev(alt_in)), dev(flags_h)
    outs = [fresh_outputs(n_out) for _ in range(40)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = torch.randn(2048, 2048, device="cuda")
        for _ in range(8):
            a = a @ a / 64.0
        for k in range(40):
            an.analyze_mixed_views(vs, d_ins[k & 1], outs[k][0], outs[k][1], outs[k][2] if k % 5 == 0 else None, d_bad_frame=d_flags, stream=s.cuda_stream)
    s.synchronize()
    blank = np.full_like(want[2], A.SENTINEL)
    for k in range(40):
        w = alt_want if k & 1 else want
        assert_outputs([t.cpu().numpy() for t in outs[k]], (w[0], w[1], w[2] if k % 5 == 0 else blank), "call %d of 40" % k)
    an.close()


def test_a_call_on_a_second_stream_right_after_one_on_the_first(the_tick, the_other_input):
    """both calls write the analyzer's columns: the second is ordered behind the first on the device"""
    descs, vs, d_in_h, flags_h, n_out, placed, want = the_tick
    torch = torch_mod()
    an = pkg.Lc3Analyzer(descs, len(vs), len(placed))
    alt_in, alt_want = the_other_input
    d_a, d_b, d_flags = dev(d_in_h), dev(alt_in), dev(flags_h)
    o1, o2, o3 = fresh_outputs(n_out), fresh_outputs(n_out), fresh_outputs(n_out)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = torch.randn(2048, 2048, device="cuda")
        for _ in range(8):
            a = a @ a / 64.0  # keeps the first stream busy: its call has not run when the second is queued
        an.analyze_mixed_views(vs, d_a, *o1, d_bad_frame=d_flags, stream=s1.cuda_stream)
    an.analyze_mixed_views(vs, d_b, *o2, d_bad_frame=d_flags, stream=s2.cuda_stream)
    an.analyze_mixed_views(vs, d_a, *o3, d_bad_frame=d_flags, stream=s1.cuda_stream)
    torch.cuda.synchronize()
    assert_outputs([t.cpu().numpy() for t in o1], want, "first stream")
    assert_outputs([t.cpu().numpy() for t in o2], alt_want, "second stream")
    assert_outputs([t.cpu().numpy() for t in o3], want, "first stream again")
    an.close()


def test_in_a_process_that_never_creates_a_codec_handle():
    code = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import inspect_lib as I
import analyze_views_lib as A
from inspect_views_lib import view, views_of
pkg = importlib.import_module("lc3-codec_amd")
data = np.array(I.clean_frames(24000, 7500, 60, 100), np.uint8)
data[::3] = I.random_frames(len(data[::3]), 60, np.random.default_rng(1))
ring = np.full(12 + 100 * 72, 0xEE, np.uint8)
for t in range(100):
    ring[12 + 72 * t: 72 + 72 * t] = data[t]
an = pkg.Lc3Analyzer([(24000, 7500, 60)], 1, 100)
d_e = torch.zeros(100, dtype=torch.float32, device="cuda")
d_b = torch.zeros((100, 64), dtype=torch.float32, device="cuda")
d_s = torch.zeros((100, 400), dtype=torch.float32, device="cuda")
an.analyze_mixed_views(views_of(view(n_frames=100, byte_off=12, byte_pitch=72)), torch.from_numpy(ring).cuda(), d_e, d_b, d_s)
torch.cuda.synchronize()
we, wb, ws = A.expected_outputs([(t, 0, bytes(data[t]), 0) for t in range(100)], [(24000, 7500, 60)], 100)
assert A.same_bits(d_e.cpu().numpy(), we) and A.same_bits(d_b.cpu().numpy(), wb) and A.same_bits(d_s.cpu().numpy(), ws)
assert 0 < (we < 0).sum() < 100
an.close()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
