"""lc3gpu_inspect_mixed_views on the GPU: the status and the record of every frame of a tick, read where the frames lie (ring slots behind
packet headers) and written where their flags lie.  Yardsticks: the oracle's records (inspect_lib: lc3o_dec_side_info + lc3o_dec_arith),
lc3gpu_inspect run per (configuration, size) on gathered copies, and lc3gpu_decode_mixed_views on a fresh decoder (its PLC count) with an
oracle decoder per stream.  After every call the WHOLE output arrays are compared, sentinels between and around the frames included."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import inspect_lib as I
from inspect_views_lib import expected_outputs, tick, view, views_of

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ECHANNEL, ELENGTH = 0, -1, -2, -3
SF, IF = 0xCC, 0x5A5A5A5A  # sentinels of the status and the record array


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
    return (torch.full((n_out,), SF, dtype=torch.uint8, device="cuda"),
            torch.from_numpy(np.full((n_out, 32), IF, np.uint32).view(np.int32)).cuda())


def run(insp, vs, d_in, d_flags, n_out, status=True, info=True, stream=None):
    """one call on fresh sentinel-filled outputs -> (status uint8[n_out], info int32[n_out][32]) as numpy"""
    d_status, d_info = fresh_outputs(n_out)
    insp.inspect_mixed_views(vs, d_in, d_status if status else None, d_info if info else None, d_bad_frame=d_flags,
                             stream=cur_stream() if stream is None else stream)
    torch_mod().cuda.synchronize()
    return d_status.cpu().numpy(), d_info.cpu().numpy()


def assert_outputs(got, want, what):
    (gs, gi), (ws, wi) = got, want
    bad = np.nonzero(gs != ws)[0]
    assert not len(bad), "%s: %d status bytes differ; first at %d: %d, expected %d" % (what, len(bad), bad[0], gs[bad[0]], ws[bad[0]])
    bad = np.nonzero((gi != wi).any(1))[0]
    assert not len(bad), "%s: %d records differ; first at %d\nexpected %s\ngpu      %s" % (what, len(bad), bad[0], wi[bad[0]].tolist(), gi[bad[0]].tolist())


@pytest.fixture(scope="module")
def the_tick():
    """about 40 frames of each of the 12 configurations, and what the call must leave (computed once, never written)"""
    descs, vs, d_in, flags, n_out, frames = tick(np.random.default_rng(777), per_config=36)
    want = expected_outputs(frames, n_out, SF, IF)
    for a in (vs, d_in, flags) + want:
        a.setflags(write=False)
    return descs, vs, d_in, flags, n_out, frames, want


def test_one_call_over_all_twelve_configurations(the_tick):
    descs, vs, d_in, flags, n_out, frames, want = the_tick
    assert len(frames) == 12 * 40 and len(set(want[0][[f[0] for f in frames]].tolist())) >= 6
    insp = pkg.Lc3Inspector(descs, len(vs))
    got = run(insp, vs, dev(d_in), dev(flags), n_out)
    assert_outputs(got, want, "the tick")
    # lc3gpu_inspect per (configuration, size) on gathered copies: byte for byte the same records
    torch = torch_mod()
    buckets = {}
    for idx, fs, us, fr, flagged in frames:
        buckets.setdefault((fs, us, len(fr)), []).append((idx, fr, flagged))
    assert len(buckets) > 40
    for (fs, us, nb), items in buckets.items():
        data = np.stack([fr for _, fr, _ in items])
        d_rec = torch.zeros((len(items), 32), dtype=torch.int32, device="cuda")
        pkg.inspect(us, fs, dev(data), d_rec, nb, len(items), d_bad_frame=dev(np.array([f for _, _, f in items], np.uint8)), stream=cur_stream())
        torch.cuda.synchronize()
        assert np.array_equal(d_rec.cpu().numpy(), got[1][[i for i, _, _ in items]]), (fs, us, nb)
    insp.close()


def test_output_forms_agree_and_leave_the_other_array_alone(the_tick):
    descs, vs, d_in, flags, n_out, frames, want = the_tick
    insp = pkg.Lc3Inspector(descs, len(vs))
    d, f = dev(d_in), dev(flags)
    s_only = run(insp, vs, d, f, n_out, info=False)
    i_only = run(insp, vs, d, f, n_out, status=False)
    assert_outputs((s_only[0], i_only[1]), want, "status only + records only")
    assert (s_only[1].view(np.uint32) == IF).all() and (i_only[0] == SF).all()
    # without flags: every frame on its own bytes
    unflagged = expected_outputs([(i, fs, us, fr, 0) for i, fs, us, fr, _ in frames], n_out, SF, IF)
    assert_outputs(run(insp, vs, d, None, n_out), unflagged, "no flags")
    # a record array that is only 4-byte aligned
    torch = torch_mod()
    raw = torch.from_numpy(np.full(n_out * 32 + 1, IF, np.uint32).view(np.int32)).cuda()
    d_status, _ = fresh_outputs(n_out)
    insp.inspect_mixed_views(vs, d, d_status, raw[1:], d_bad_frame=f, stream=cur_stream())
    torch.cuda.synchronize()
    assert raw.data_ptr() % 16 == 0 and raw[0].item() == np.array([IF], np.uint32).view(np.int32)[0]
    assert_outputs((d_status.cpu().numpy(), raw[1:].cpu().numpy().reshape(n_out, 32)), want, "records at a 4-byte aligned address")
    insp.close()


def _simple_tick(specs, rng, slot_pitch=412):
    """specs: (fs, us, nbytes, n_frames) per view, one stream each; half clean, half damaged or random bytes; flags on a few"""
    descs, vs, slots, frames = [], [], [], []
    out_idx = 1
    for ch, (fs, us, nb, T) in enumerate(specs):
        descs.append((fs, us, nb))
        fr = I.clean_frames(fs, us, nb, T, seed=ch + 1) if nb >= 20 else I.random_frames(T, nb, rng)
        fr = np.array(fr, np.uint8)
        hit = rng.random(T) < 0.4
        fr[hit] = I.random_frames(int(hit.sum()), nb, rng)
        vs.append(view(channel=ch, n_frames=T, byte_off=12 + slot_pitch * len(slots), byte_pitch=slot_pitch, flag_off=out_idx, flag_pitch=2))
        for t in range(T):
            flagged = int(rng.random() < 0.05)
            slots.append(fr[t])
            frames.append((out_idx + 2 * t, fs, us, fr[t], flagged))
        out_idx += 2 * T + 1
    d_in = np.full(len(slots) * slot_pitch + 12, 0xEE, np.uint8)
    for k, fr in enumerate(slots):
        d_in[12 + slot_pitch * k: 12 + slot_pitch * k + len(fr)] = fr
    flags = np.ones(out_idx + 2, np.uint8)
    for idx, _, _, _, flagged in frames:
        flags[idx] = flagged
    return descs, views_of(*vs), d_in, flags, out_idx + 2, frames


@pytest.mark.parametrize("delta", [None, -1, 0, 1])
def test_frame_counts_around_the_workgroup_size(delta):
    """1, fpb - 1, fpb and fpb + 1 frames in all, with fpb read from the plan; 8 kHz streams among them"""
    fpb, lds, slots = api.inspector_plan_info(40)
    assert fpb == 128 and lds <= 65536 and slots >= 2
    total = 1 if delta is None else fpb + delta
    rng = np.random.default_rng(100 + total)
    specs = [(8000, 7500, 40, total)] if total < 3 else [(8000, 7500, 40, total - 2), (8000, 7500, 40, 2)]
    descs, vs, d_in, flags, n_out, frames = _simple_tick(specs, rng)
    insp = pkg.Lc3Inspector(descs, 4)
    assert_outputs(run(insp, vs, dev(d_in), dev(flags), n_out), expected_outputs(frames, n_out, SF, IF), "%d frames" % total)
    insp.close()


def test_two_buckets_that_each_cross_a_workgroup_border_and_the_edge_sizes():
    fpb400 = api.inspector_plan_info(400)[0]
    assert fpb400 == 64
    rng = np.random.default_rng(5)
    # with a 400-byte frame in the call a workgroup has 64 lanes: 70 + 7 frames of one bucket and 65 + 66 of another cross a border each
    specs = [(48000, 10000, 150, 70), (8000, 10000, 20, 65), (48000, 10000, 150, 7), (8000, 10000, 20, 66), (44100, 7500, 400, 3),
             (8000, 7500, 1, 5), (16000, 10000, 6, 5), (24000, 7500, 7, 5), (32000, 10000, 20, 5), (8000, 7500, 400, 2)]
    descs, vs, d_in, flags, n_out, frames = _simple_tick(specs, rng)
    insp = pkg.Lc3Inspector(descs, len(vs))
    want = expected_outputs(frames, n_out, SF, IF)
    assert_outputs(run(insp, vs, dev(d_in), dev(flags), n_out), want, "edge shapes")
    # the same frames without the 400-byte ones: 128 or 256 lanes per workgroup
    keep = [k for k, s in enumerate(specs) if s[2] != 400]
    sub = views_of(*[vs[k: k + 1] for k in keep])
    kept = [f for f in frames if len(f[3]) != 400]
    assert_outputs(run(insp, sub, dev(d_in), dev(flags), n_out), expected_outputs(kept, n_out, SF, IF), "edge shapes, wider workgroups")
    insp.close()


def test_status_is_what_decode_mixed_views_conceals():
    """the same descriptors, views, bytes and flags through lc3gpu_decode_mixed_views on a fresh decoder: as many PLC events as non-zero
    statuses; an oracle decoder per stream agrees frame by frame"""
    torch = torch_mod()
    rng = np.random.default_rng(31)
    specs = [(fs, us, nb, T) for (fs, us), nb, T in zip(I.CONFIGS * 2, [40, 57, 150, 20, 80, 400, 33, 100] * 3, [1, 3, 4, 2, 5, 1] * 4)]
    descs, vs, d_in, flags, n_out, frames = _simple_tick(specs, rng)
    vs = vs.copy()
    pcm_at = 0
    for k, (fs, us, nb, T) in enumerate(specs):  # the PCM placement the decode call needs; the inspector does not look at it
        vs[k]["pcm_stride"], vs[k]["pcm_off"] = 1, pcm_at
        pcm_at += T * I.config(fs, us).nf
    insp = pkg.Lc3Inspector(descs, len(vs))
    status, info = run(insp, vs, dev(d_in), dev(flags), n_out)
    assert_outputs((status, info), expected_outputs(frames, n_out, SF, IF), "decode equivalence")
    at = np.array([f[0] for f in frames])
    lost = status[at] != 0
    assert 0 < lost.sum() < len(frames)
    dec = pkg.Lc3Decoder.mixed(descs)
    before = dec.plc_events()
    d_pcm = torch.zeros(pcm_at, dtype=torch.int16, device="cuda")
    dec.decode_mixed_views(vs, dev(d_in), d_pcm, stream=cur_stream(), d_bad_frame=dev(flags))
    torch.cuda.synchronize()
    assert dec.plc_events() - before == lost.sum()
    assert dec.pair_timeouts() == 0
    dec.close()
    k = 0
    for fs, us, nb, T in specs:
        data = np.stack([frames[k + t][3] for t in range(T)])
        bad = np.array([frames[k + t][4] for t in range(T)], np.uint8)
        assert np.array_equal(I.oracle_plc(fs, us, data, None, bad), lost[k: k + T]), (fs, us, nb)
        k += T
    insp.close()


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
    frames = [(s, fs, us, fr[t], int(flags[s])) for t, s in enumerate(order)]
    insp = pkg.Lc3Inspector([(fs, us, nb)], 2)
    assert_outputs(run(insp, vs, dev(ring), dev(flags), SLOTS), expected_outputs(frames, SLOTS, SF, IF), "ring wrap")
    insp.close()


def test_every_refusal_on_a_live_inspector_leaves_the_outputs_alone(the_tick):
    descs, vs, d_in_h, flags_h, n_out, frames, want = the_tick
    torch = torch_mod()
    L = pkg.load_library()
    insp = pkg.Lc3Inspector(descs, len(vs))
    d_in, d_flags = dev(d_in_h), dev(flags_h)
    d_status, d_info = fresh_outputs(n_out)
    one = view(channel=3, n_frames=4, byte_off=12, byte_pitch=412, flag_off=5, flag_pitch=2)
    P = lambda a: a.ctypes.data_as(api.ctypes.c_void_p)

    def call(v, n=None, insp_h=insp._h, din=d_in.data_ptr(), in_bytes=d_in.numel(), fl=d_flags.data_ptr(), n_flags=n_out, st=d_status.data_ptr(),
             n_status=n_out, inf=d_info.data_ptr(), n_info=n_out):
        return L.lc3gpu_inspect_mixed_views(insp_h, None if v is None else P(v), len(v) if n is None else n, din, in_bytes, fl, n_flags, st, n_status,
                                            inf, n_info, cur_stream())

    nb3 = 57
    refused = [
        (call(views_of(view(channel=-1))), ECHANNEL), (call(views_of(view(channel=12))), ECHANNEL),
        (call(views_of(view(n_frames=0))), ELENGTH), (call(views_of(view(nbytes=401))), ELENGTH), (call(views_of(view(nbytes=-1))), ELENGTH),
        (call(views_of(view(n_frames=2**31 - 1, nbytes=1), view(n_frames=1, nbytes=1))), ELENGTH),
        (call(views_of(*([one] * (len(vs) + 1)))), ELENGTH),
        (call(views_of(view(n_frames=3, byte_off=d_in.numel() - 2 * 412 - nb3 + 1, byte_pitch=412))), ELENGTH),
        (call(views_of(view(n_frames=3, flag_off=7, flag_pitch=5)), n_flags=17), ELENGTH),
        (call(views_of(view(n_frames=3, flag_off=7, flag_pitch=5)), n_status=17), ELENGTH),
        (call(views_of(view(n_frames=3, flag_off=7, flag_pitch=5)), n_info=17), ELENGTH),
        (call(views_of(view(byte_off=-1))), EINVAL), (call(views_of(view(flag_off=-1))), EINVAL),
        (call(views_of(view(n_frames=2, byte_pitch=nb3 - 1))), EINVAL), (call(views_of(view(n_frames=2, flag_pitch=-1))), EINVAL),
        (call(views_of(view(reserved=(0, 0, 1)))), EINVAL),
        (call(views_of(one), st=None, inf=None), EINVAL), (call(views_of(one), insp_h=None), EINVAL), (call(None, n=1), EINVAL),
        (call(views_of(one), din=None), EINVAL), (call(views_of(one), n=-1), EINVAL),
        (call(views_of(one), inf=d_info.data_ptr() + 2), EINVAL),
        (call(views_of(one), st=d_in.data_ptr() + 100), EINVAL), (call(views_of(one), st=d_flags.data_ptr()), EINVAL),
        (call(views_of(one), st=d_info.data_ptr() + 128, n_status=64), EINVAL), (call(views_of(one), inf=d_in.data_ptr(), n_info=4), EINVAL),
        (call(views_of(one), inf=d_flags.data_ptr(), n_info=1), EINVAL),
    ]
    torch.cuda.synchronize()
    for k, (rc, code) in enumerate(refused):
        assert rc == code, (k, rc, code)
    assert (d_status.cpu().numpy() == SF).all() and (d_info.cpu().numpy().view(np.uint32) == IF).all()
    # accepted right at the ends, and no views at all
    assert call(views_of(view(n_frames=3, byte_off=d_in.numel() - 2 * 412 - nb3, byte_pitch=412, flag_off=n_out - 11, flag_pitch=5))) == OK
    assert call(vs[:0]) == OK
    torch.cuda.synchronize()
    assert (d_status.cpu().numpy() != SF).sum() == 3
    # the inspector still works
    assert_outputs(run(insp, vs, d_in, d_flags, n_out), want, "after the refusals")
    insp.close()


def test_forty_calls_queued_back_to_back_each_with_its_own_views(the_tick):
    """more calls in flight than the upload ring has slots, behind a kernel that keeps the stream busy; the view array is reused at once"""
    descs, vs, d_in_h, flags_h, n_out, frames, want = the_tick
    torch = torch_mod()
    slots = api.inspector_plan_info(400)[2]
    assert slots < 40
    insp = pkg.Lc3Inspector(descs, len(vs))
    d_in, d_flags = dev(d_in_h), dev(flags_h)
    outs, subsets = [fresh_outputs(n_out) for _ in range(40)], []
    rng = np.random.default_rng(40)
    scratch = vs.copy()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = torch.randn(2048, 2048, device="cuda")
        for _ in range(8):
            a = a @ a / 64.0
        for k in range(40):
            pick = np.sort(rng.choice(len(vs), int(rng.integers(1, len(vs))), replace=False))
            subsets.append(pick)
            scratch[: len(pick)] = vs[pick]
            insp.inspect_mixed_views(scratch[: len(pick)], d_in, outs[k][0], outs[k][1], d_bad_frame=d_flags, stream=s.cuda_stream)
            scratch[:] = vs[0]  # (the list may be reused as soon as the call returns)
    s.synchronize()
    # which output index belongs to which view: a view's frames are its flag_off + t * pitch
    for k, pick in enumerate(subsets):
        ws, wi = np.full(n_out, SF, np.uint8), np.full((n_out, 32), IF, np.uint32).view(np.int32)
        for v in vs[pick]:
            for t in range(int(v["n_frames"])):
                i = int(v["flag_off"]) + t * (int(v["flag_pitch"]) or 1)
                ws[i], wi[i] = want[0][i], want[1][i]
        assert_outputs((outs[k][0].cpu().numpy(), outs[k][1].cpu().numpy()), (ws, wi), "call %d of 40" % k)
    insp.close()


def test_ordered_behind_a_kernel_that_writes_the_input(the_tick):
    descs, vs, d_in_h, flags_h, n_out, frames, want = the_tick
    torch = torch_mod()
    insp = pkg.Lc3Inspector(descs, len(vs))
    key = 0x5A
    d_src, d_flags = dev(d_in_h ^ np.uint8(key)), dev(flags_h)
    d_in = torch.zeros(d_in_h.size, dtype=torch.uint8, device="cuda")
    d_status, d_info = fresh_outputs(n_out)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = torch.randn(2048, 2048, device="cuda")
        for _ in range(8):
            a = a @ a / 64.0  # keeps the stream busy before the writing kernel
        torch.bitwise_xor(d_src, key, out=d_in)
        insp.inspect_mixed_views(vs, d_in, d_status, d_info, d_bad_frame=d_flags, stream=s.cuda_stream)
    s.synchronize()
    assert_outputs((d_status.cpu().numpy(), d_info.cpu().numpy()), want, "stream order")
    insp.close()


def test_in_a_process_that_never_creates_a_codec_handle():
    code = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import inspect_lib as I
from inspect_views_lib import expected_outputs, view, views_of
pkg = importlib.import_module("lc3-codec_amd")
data = np.array(I.clean_frames(24000, 7500, 60, 100), np.uint8)
data[::3] = I.random_frames(len(data[::3]), 60, np.random.default_rng(1))
ring = np.full(12 + 100 * 72, 0xEE, np.uint8)
for t in range(100):
    ring[12 + 72 * t: 72 + 72 * t] = data[t]
insp = pkg.Lc3Inspector([(24000, 7500, 60)], 1)
d_status = torch.full((100,), 0xCC, dtype=torch.uint8, device="cuda")
d_info = torch.zeros((100, 32), dtype=torch.int32, device="cuda")
insp.inspect_mixed_views(views_of(view(n_frames=100, byte_off=12, byte_pitch=72)), torch.from_numpy(ring).cuda(), d_status, d_info)
torch.cuda.synchronize()
ws, wi = expected_outputs([(t, 24000, 7500, data[t], 0) for t in range(100)], 100)
assert np.array_equal(d_info.cpu().numpy(), wi) and np.array_equal(d_status.cpu().numpy(), ws)
insp.close()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
