"""lc3gpu_mix_mixed_views on the GPU: the room mixes of a tick, the PCM read where it lies in one ring array and written where it belongs in
another.  The yardstick is the numpy model of the header's three formulas (mix_lib); after every call the WHOLE output array is compared
with it, the sentinels between and around the views included.  The shapes are those of tests/test_emu_mix_views.py (shape_ticks), which
states why each is there."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import mix_lib as M
from mix_lib import mix_ins, mix_outs, view, views_of
from test_emu_mix_views import CH8S, CH48, CH48S, saturation_tick, shape_ticks

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("lc3-codec_amd")
api = importlib.import_module("lc3-codec_amd.api")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ECHANNEL, ELENGTH = 0, -1, -2, -3


def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch


def dev(a):
    return torch_mod().from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared fixtures are read-only)


def cur_stream():
    return torch_mod().cuda.current_stream().cuda_stream


def run(mx, t, stream=None, pcm_in=None):
    """one call on a fresh sentinel-filled output ring -> the whole ring as numpy"""
    d_in, d_out = dev(t.pcm_in if pcm_in is None else pcm_in), dev(t.pcm_out)
    mx.mix_mixed_views(t.in_views, t.ins, d_in if len(t.in_views) else None, t.out_views, t.outs, d_out, stream=cur_stream() if stream is None else stream)
    torch_mod().cuda.synchronize()
    return d_out.cpu().numpy()


def assert_ring(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: %d samples differ; first at %d\nexpected %s\ngpu      %s" % (what, len(bad), bad[0], want[bad[:8]], got[bad[:8]])


@pytest.fixture(scope="module")
def ticks():
    return shape_ticks()


@pytest.mark.parametrize("name", ["frame lengths, frame counts, strides and pitches", "four 7.5 ms frames with three 10 ms frames",
                                  "sample counts around the workgroup's", "room sizes", "one input view feeding two buses",
                                  "24 buses of different sizes", "rounding"])
def test_the_shapes_bit_for_bit_with_the_ring_around_them(ticks, name):
    t = ticks[name]
    mx = pkg.Lc3Mixer(t.descs, t.max_views)
    assert_ring(run(mx, t), t.want, name)
    mx.close()


def test_the_shapes_are_the_ones_the_contract_names(ticks):
    """what the parametrised test above relies on: no GPU work here beyond the plan's figures"""
    spw = api.mixer_plan_info()[0]
    S = lambda t: {int(v["n_frames"]) * M.nf_of(*t.descs[int(v["channel"])][:2]) for v in t.out_views}
    got = S(ticks["sample counts around the workgroup's"])
    assert {2 * spw - 4, 5 * spw, 13 * spw + 4} <= got  # (S mod 512 is a multiple of 4: - 2 and + 2 do not exist)
    t = ticks["frame lengths, frame counts, strides and pitches"]
    assert {(M.nf_of(*t.descs[int(v["channel"])][:2]), int(v["n_frames"])) for v in t.out_views} == {(nf, n) for nf in (60, 80, 360, 480) for n in (1, 3)}
    assert {int(v["pcm_stride"]) for v in t.out_views} == {1, 2, 8} == {int(v["pcm_stride"]) for v in t.in_views}
    assert {0} < {int(v["pcm_pitch"]) for v in t.out_views} and {0} < {int(v["pcm_pitch"]) for v in t.in_views}
    t = ticks["24 buses of different sizes"]
    assert len(set(t.outs["bus"].tolist())) >= 20
    t = ticks["room sizes"]
    sizes = sorted(int((t.ins["bus"] == b).sum()) for b in set(t.outs["bus"].tolist()))
    assert sizes == [0, 1, 2, 3, 65]
    t = ticks["rounding"]
    assert t.want[M.sample_index(t.out_views[0], t.descs)][:6].tolist() == [1, 0, -1, 2, 16384, -16384]


@pytest.mark.parametrize("value,gain,total", [(-32768, -32768, 2**30), (32767, 32767, 1073676288)])
def test_16384_inputs_on_one_bus_saturate(value, gain, total):
    t = saturation_tick(value, gain, np.random.default_rng(4))
    assert 16384 * ((value * gain + 8192) >> 14) == total
    mx = pkg.Lc3Mixer(t.descs, t.max_views)
    got = run(mx, t)
    assert_ring(got, t.want, "saturation")
    for v in t.out_views:  # (with the minus term too: the total lies far above the clamp)
        assert (got[M.sample_index(v, t.descs)] == 32767).all()
    mx.close()


def test_clamp_share_of_full_range_rooms_of_three():
    """rooms of three full-range uniform inputs at unity gain, N-1 outputs plus one listen-only output per room: between 15 and 40 % of the
    model's output samples lie on the clamp, so both branches carry weight before the device result is compared"""
    rng = np.random.default_rng(6)
    t = M.make_tick([M.n_minus_one_room([CH48] * 3, rng, listen=True) for _ in range(8)], rng)
    vals = np.concatenate([t.want[M.sample_index(v, t.descs)] for v in t.out_views])
    share = float(((vals == 32767) | (vals == -32768)).mean())
    print("clamp share %.4f" % share)
    assert 0.15 <= share <= 0.40, share
    mx = pkg.Lc3Mixer(t.descs, t.max_views)
    assert_ring(run(mx, t), t.want, "clamp share")
    mx.close()


def test_a_tick_through_decode_mix_and_encode_is_decode_the_model_and_encode():
    """the ten encodable configurations in rooms of 2 to 5 (one room per rate, 7.5 and 10 ms participants side by side: four frames against
    three): lc3gpu_decode_mixed_views, the mix, lc3gpu_encode_mixed_views on the tick's own two view arrays, against decode, mix_lib on
    the downloaded ring, encode -- byte for byte, state blobs included"""
    torch = torch_mod()
    rng = np.random.default_rng(8)
    synth = importlib.import_module("lc3-codec_amd.synth")
    rates, sizes = (16000, 24000, 32000, 44100, 48000), (2, 3, 4, 5, 3)
    parts = [(fs, (7500, 10000)[(k + r) & 1], r) for r, (fs, n) in enumerate(zip(rates, sizes)) for k in range(n)]
    assert {(fs, us) for fs, us, _ in parts} == {(fs, us) for fs in rates for us in (7500, 10000)}
    descs = [(fs, us, 40 + 10 * (k % 4)) for k, (fs, us, _) in enumerate(parts)]
    T = lambda us: 4 if us == 7500 else 3
    # what every participant sent: its own encoder's frames of a synthetic signal, in ring slots of 412 bytes behind a 12-byte header
    src = pkg.Lc3Encoder.mixed(descs)
    ring_a, ring_b, byte_pos = M._Ring(rng), M._Ring(rng), 12
    dviews, eviews, sviews, pcm_src, pos = [], [], [], [], 0
    for k, (fs, us, _) in enumerate(parts):
        nf, n = M.nf_of(fs, us), T(us)
        x = synth.make_pcm(1, n, nf, fs)[0].reshape(-1).astype(np.int16)
        x = np.clip(x.astype(np.int64) * 3 + rng.integers(-2000, 2001, x.size), -32768, 32767).astype(np.int16)  # (loud: the mixes reach the clamp)
        sviews.append(view(channel=k, n_frames=n, pcm_off=pos, byte_off=byte_pos, byte_pitch=412))
        pcm_src.append(x)
        pos += x.size
        dv = ring_a.place(k, n, int(rng.choice([1, 1, 2])), int(rng.choice([0, 6])), descs)
        ev = ring_b.place(k, n, int(rng.choice([1, 1, 2])), int(rng.choice([0, 6])), descs)
        dv[0]["byte_off"], dv[0]["byte_pitch"] = byte_pos, 412
        ev[0]["byte_off"], ev[0]["byte_pitch"] = byte_pos, 412
        dviews.append(dv), eviews.append(ev)
        byte_pos += n * 412
    sviews, dviews, eviews = views_of(*sviews), views_of(*dviews), views_of(*eviews)
    d_sent = torch.full((byte_pos + 7,), 0xEE, dtype=torch.uint8, device="cuda")
    src.encode_mixed_views(sviews, dev(np.concatenate(pcm_src)), d_sent)
    ins = mix_ins(*[(r, M.UNITY if k % 3 else 12000) for k, (_, _, r) in enumerate(parts)])
    outs = mix_outs(*[(r, k) for k, (_, _, r) in enumerate(parts)])  # N-1: everybody hears the others
    ring_in = np.full(ring_a.cursor + 8, M.SENTINEL, np.int16)
    ring_out = np.full(ring_b.cursor + 8, M.SENTINEL, np.int16)

    def tick(mix):
        dec, enc = pkg.Lc3Decoder.mixed(descs), pkg.Lc3Encoder.mixed(descs)
        d_pcm, d_cap = dev(ring_in), dev(ring_out)
        d_back = torch.full((byte_pos + 7,), 0xEE, dtype=torch.uint8, device="cuda")
        dec.decode_mixed_views(dviews, d_sent, d_pcm)
        d_cap = mix(d_pcm, d_cap)
        enc.encode_mixed_views(eviews, d_cap, d_back)
        torch.cuda.synchronize()
        res = (d_back.cpu().numpy(), enc.state_save(), dec.state_save(), d_pcm.cpu().numpy(), d_cap.cpu().numpy())
        dec.close(), enc.close()
        return res

    mx = pkg.Lc3Mixer(descs, len(parts) * 2)

    def in_place(d_pcm, d_cap):
        mx.mix_mixed_views(dviews, ins, d_pcm, eviews, outs, d_cap)
        return d_cap

    def by_the_model(d_pcm, d_cap):
        torch.cuda.synchronize()
        return dev(M.model(descs, dviews, ins, d_pcm.cpu().numpy(), eviews, outs, ring_out))

    got, want = tick(in_place), tick(by_the_model)
    for name, g, w in zip(("the bytes sent back", "the encoder's state", "the decoder's state", "the playout ring", "the capture ring"), got, want):
        assert np.array_equal(g, w), name
    # not a copy: in a room of three or more every output differs from every input of the tick somewhere (in a room of two at unity gain
    # the N-1 mix IS the other participant's samples)
    cap, pcm = got[4], got[3]
    mixed = 0
    for o, ev in enumerate(eviews):
        if sizes[parts[o][2]] < 3:
            continue
        mine = cap[M.sample_index(ev, descs)]
        for dv in dviews:
            other = pcm[M.sample_index(dv, descs)]
            assert len(other) != len(mine) or (other != mine).any(), o
        mixed += 1
    assert mixed == sum(n for n in sizes if n >= 3) == 15
    assert (got[0] != 0xEE).sum() >= sum(T(us) * 40 for _, us, _ in parts)
    mx.close(), src.close()


def test_every_refusal_on_a_live_mixer_leaves_the_output_ring_alone(ticks):
    t = ticks["room sizes"]
    torch = torch_mod()
    L = pkg.load_library()
    n_views = len(t.in_views) + len(t.out_views)
    mx = pkg.Lc3Mixer(t.descs, n_views)
    d_in, d_out = dev(t.pcm_in), dev(t.pcm_out)
    P = lambda a: None if a is None else a.ctypes.data_as(api.ctypes.c_void_p)
    i1, o1 = view(channel=CH48, n_frames=3, pcm_off=10), view(channel=CH48S, n_frames=4, pcm_off=20)
    keep = []

    def call(vin=(i1,), tin=((0, M.UNITY),), vout=(o1,), tout=((0, 0),), h=mx._h, n_in=None, n_out=None, din=d_in.data_ptr(), in_elems=d_in.numel(),
             dout=d_out.data_ptr(), out_elems=d_out.numel(), null=()):
        a = [views_of(*vin), mix_ins(*tin), views_of(*vout), mix_outs(*tout)]
        keep.append(a)
        ni, no = len(a[0]) if n_in is None else n_in, len(a[2]) if n_out is None else n_out
        p = [None if k in null else P(a[k]) for k in range(4)]
        return L.lc3gpu_mix_mixed_views(h, p[0], p[1], ni, din, in_elems, p[2], p[3], no, dout, out_elems, cur_stream())

    assert d_in.numel() > 1500 and d_out.numel() > 1500 and n_views >= 70
    many = [i1] * (n_views + 1)
    refused = [
        (call(vin=(view(channel=-1),)), ECHANNEL), (call(vout=(view(channel=12),)), ECHANNEL),
        (call(vin=(view(channel=CH48, n_frames=0),)), ELENGTH), (call(vout=(view(channel=CH48, n_frames=-1),)), ELENGTH),
        (call(vin=(view(channel=CH48, n_frames=4473925),)), ELENGTH),
        (call(in_elems=10 + 1439), ELENGTH), (call(out_elems=20 + 1439), ELENGTH),
        (call(vin=(view(channel=CH48, n_frames=3, pcm_off=d_in.numel() - 1438),)), ELENGTH),
        (call(vout=(view(channel=CH48S, n_frames=4, pcm_off=d_out.numel() - 1438),)), ELENGTH),
        (call(vin=many, tin=[(0, 1)] * len(many)), ELENGTH),
        (call(vout=(view(channel=CH48S, n_frames=3),)), ELENGTH), (call(vin=(i1, view(channel=CH48, n_frames=2)), tin=((0, 1), (0, 1))), ELENGTH),
        (call(vin=(view(channel=M.channel_of(44100, 10000), n_frames=3),)), EINVAL),
        (call(tin=((n_views, 1),), tout=((0, -1),)), EINVAL), (call(tout=((n_views, -1),)), EINVAL), (call(tout=((-1, -1),)), EINVAL),
        (call(tin=((0, 32768),)), EINVAL), (call(tin=((0, -32769),)), EINVAL),
        (call(tout=((0, 1),)), EINVAL), (call(tout=((0, -2),)), EINVAL), (call(vin=(i1, i1), tin=((0, 1), (1, 1)), tout=((0, 1),)), EINVAL),
        (call(vin=(view(channel=CH48, n_frames=3, pcm_stride=0),)), EINVAL), (call(vout=(view(channel=CH48, n_frames=3, pcm_stride=9),)), EINVAL),
        (call(vin=(view(channel=CH48, n_frames=3, pcm_off=-2),)), EINVAL), (call(vout=(view(channel=CH48, n_frames=3, pcm_pitch=478),)), EINVAL),
        (call(vout=(view(channel=CH48, n_frames=3, reserved=(0, 1, 0)),)), EINVAL),
        (call(vin=(view(channel=CH48, n_frames=3, pcm_off=11),)), EINVAL), (call(vout=(view(channel=CH48, n_frames=3, pcm_pitch=481),)), EINVAL),
        (call(din=d_in.data_ptr() + 2), EINVAL), (call(dout=d_out.data_ptr() + 2), EINVAL),
        (call(vout=(view(channel=CH48, n_frames=3, pcm_stride=2),), dout=d_out.data_ptr() + 1), EINVAL),
        (call(dout=d_in.data_ptr() + 4096, out_elems=1500), EINVAL), (call(din=d_out.data_ptr(), in_elems=1500), EINVAL),
        (call(dout=d_in.data_ptr() + 2 * d_in.numel() - 4, out_elems=1500), EINVAL),
        (call(h=None), EINVAL), (call(null=(0,)), EINVAL), (call(null=(1,)), EINVAL), (call(null=(2,)), EINVAL), (call(null=(3,)), EINVAL),
        (call(din=None), EINVAL), (call(dout=None), EINVAL), (call(n_in=-1), EINVAL), (call(n_out=-1), EINVAL),
    ]
    torch.cuda.synchronize()
    for k, (rc, code) in enumerate(refused):
        assert rc == code, (k, rc, code)
    assert np.array_equal(d_out.cpu().numpy(), t.pcm_out)
    # accepted right at the ends, with no outputs (nothing launched), and with no inputs (zeros)
    assert call(vout=(), tout=()) == OK
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), t.pcm_out)
    last_in, last_out = view(channel=CH48, n_frames=3, pcm_off=d_in.numel() - 1440), view(channel=CH48S, n_frames=4, pcm_off=d_out.numel() - 1440)
    assert call(vin=(last_in,), vout=(last_out,), tout=((0, -1),)) == OK
    assert call(vin=(), tin=(), vout=(view(channel=CH8S, pcm_off=0),), tout=((3, -1),), din=None, in_elems=0, null=(0, 1)) == OK
    torch.cuda.synchronize()
    got, w = d_out.cpu().numpy(), t.pcm_out.copy()
    w[-1440:] = t.pcm_in[-1440:]
    w[:60] = 0
    assert_ring(got, w, "at the ends")
    # the mixer still works
    assert_ring(run(mx, t), t.want, "after the refusals")
    mx.close()


def test_forty_calls_queued_back_to_back_with_alternating_inputs_and_room_tables(ticks):
    """more calls in flight than the upload ring has slots, behind a kernel that keeps the stream busy: even calls mix the tick, odd calls
    another input ring under other gains and other minus inputs; every call's result is its own"""
    t = ticks["frame lengths, frame counts, strides and pitches"]
    torch = torch_mod()
    assert api.mixer_plan_info()[2] < 40
    rng = np.random.default_rng(11)
    alt_in = rng.integers(-32768, 32768, len(t.pcm_in)).astype(np.int16)
    alt_ins = t.ins.copy()
    alt_ins["gain_q14"] = rng.integers(-32768, 32768, len(alt_ins))
    alt_outs = t.outs.copy()
    for o in range(len(alt_outs)):  # another input of the same bus, or none
        same = np.nonzero(t.ins["bus"] == alt_outs["bus"][o])[0]
        alt_outs["minus"][o] = int(rng.choice(np.concatenate([same, [-1]])))
    alt_want = M.model(t.descs, t.in_views, alt_ins, alt_in, t.out_views, alt_outs, t.pcm_out)
    assert (alt_want != t.want).sum() > 1000
    mx = pkg.Lc3Mixer(t.descs, t.max_views)
    d_ins = (dev(t.pcm_in), dev(alt_in))
    rings = [dev(t.pcm_out) for _ in range(40)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = torch.randn(2048, 2048, device="cuda")
        for _ in range(8):
            a = a @ a / 64.0
        for k in range(40):
            mx.mix_mixed_views(t.in_views, alt_ins if k & 1 else t.ins, d_ins[k & 1], t.out_views, alt_outs if k & 1 else t.outs, rings[k], stream=s.cuda_stream)
    s.synchronize()
    for k in range(40):
        assert_ring(rings[k].cpu().numpy(), alt_want if k & 1 else t.want, "call %d of 40" % k)
    mx.close()


def test_a_call_on_a_second_stream(ticks):
    t = ticks["four 7.5 ms frames with three 10 ms frames"]
    torch = torch_mod()
    mx = pkg.Lc3Mixer(t.descs, t.max_views)
    d_in, o1, o2 = dev(t.pcm_in), dev(t.pcm_out), dev(t.pcm_out)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    mx.mix_mixed_views(t.in_views, t.ins, d_in, t.out_views, t.outs, o1, stream=s1.cuda_stream)
    mx.mix_mixed_views(t.in_views, t.ins, d_in, t.out_views, t.outs, o2, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert_ring(o1.cpu().numpy(), t.want, "first stream")
    assert_ring(o2.cpu().numpy(), t.want, "second stream")
    mx.close()


def test_in_a_process_that_creates_only_a_mixer():
    code = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import mix_lib as M
pkg = importlib.import_module("lc3-codec_amd")
rng = np.random.default_rng(2)
t = M.make_tick([M.n_minus_one_room([M.channel_of(32000, 10000)] * 4, rng, listen=True), M.n_minus_one_room([M.channel_of(16000, 7500)] * 2, rng)], rng)
mx = pkg.Lc3Mixer(t.descs, t.max_views)
d_out = torch.from_numpy(t.pcm_out.copy()).cuda()
mx.mix_mixed_views(t.in_views, t.ins, torch.from_numpy(t.pcm_in.copy()).cuda(), t.out_views, t.outs, d_out)
torch.cuda.synchronize()
assert (t.want != t.pcm_out).sum() > 1500  # (1840 output samples)
assert np.array_equal(d_out.cpu().numpy(), t.want)
mx.close()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
