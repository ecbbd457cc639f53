#!/usr/bin/env python3
"""lc3gpu_mix_mixed_views against what a caller does today for the room mixes of a tick in rings: per configuration a torch gather out of
the playout rings into compact int32 [members, S], an index_add per room, a subtract, a clamp and a scatter into the capture rings.  Both
routes leave the same capture rings, bit for bit: asserted before anything is timed.
The stream mix of profiles/r06_mixed_batch.json without its two 8 kHz entries (a tick is decoded AND encoded), `--frames` frames per tick
in two shapes -- streams x 1 frame and a quarter of the streams x 4 frames --, rooms of 2, 4 and 8 streams of one configuration with N-1
outputs at unity gain, PCM rings of 8 slots of 480 samples per stream (tools/views_batch.py), one process, one caller stream, GPU events
over `--steps` calls per measurement, the two routes alternating over `--rounds` rounds.  One JSON line per figure, written to `--out`
(default profiles/mix_views_measurements.jsonl) and printed:
  mix_route    today's route against ONE mixer call: ms per call of both, the ratio, the yardstick's own spread between rounds, the bytes a
               call must move at the least -- (n_in + 2 * n_out) * S * 2: every input read once, and once more as its output's minus input
               (a cache hit at best), every output written -- and that figure over the time against the copy figure of
               profiles/r04_valu_ceiling.json (bench.py's measured_copy_GBs: bytes read plus bytes written);
  whole_tick   lc3gpu_decode_mixed_views, the mix, lc3gpu_encode_mixed_views against decode plus encode without a mix (rooms of 4): what the
               middle step costs a mixing server.
usage: python tools/mix_views_batch.py [--frames 65536] [--steps 50] [--rounds 3] [--out FILE]"""
import importlib, json, os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIXED = [(16000, 10000, 40), (24000, 10000, 60), (32000, 10000, 80), (44100, 10000, 110), (48000, 10000, 150),
         (16000, 7500, 30), (24000, 7500, 45), (32000, 7500, 60), (44100, 7500, 83), (48000, 7500, 113)]
SLOTS, HEADER, SLOT_BYTES, SLOT_PCM = 8, 12, 400, 480
PITCH = HEADER + SLOT_BYTES


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    total, steps, rounds = arg("--frames", 65536), arg("--steps", 50), arg("--rounds", 3)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mix_views_measurements.jsonl")
    cmd = "python tools/mix_views_batch.py --frames %d --steps %d --rounds %d" % (total, steps, rounds)
    open(out_path, "w").close()  # a run replaces the file
    import torch

    pkg = importlib.import_module("lc3-codec_amd")
    api = importlib.import_module("lc3-codec_amd.api")
    st = torch.cuda.current_stream().cuda_stream
    nf = [pkg.Lc3Config(fs, us).nf for fs, us, _ in MIXED]
    P = api._ptr
    L = pkg.load_library()
    with open(os.path.join(ROOT, "profiles", "r04_valu_ceiling.json")) as f:
        copy_gbs = float(json.load(f)["copy"]["GBs_read_plus_write"])  # (bench.py's measured_copy_GBs: bytes read plus bytes written over time)

    def emit(**row):
        row["command"] = cmd
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")

    def events(call):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps  # ms per call

    def alternate(yard, new):
        for _ in range(3):
            yard()
            new()
        y, n = [], []
        for _ in range(rounds):
            y.append(events(yard))
            n.append(events(new))
        return y, n

    nq = len(MIXED)
    for streams_total, T in ((total, 1), (total // 4, 4)):
        per = streams_total // nq // 8 * 8  # (whole rooms of 8, 4 and 2)
        cfg_of = [q for q in range(nq) for _ in range(per)]
        desc = [MIXED[q] for q in cfg_of]
        n_ch = len(desc)
        frames = n_ch * T
        rng = np.random.default_rng(5)
        slot0 = rng.integers(0, SLOTS - T + 1, n_ch)
        first = np.arange(n_ch) * SLOTS + slot0  # first ring slot of every stream's frames
        ring_pcm, ring_rows = n_ch * SLOTS * SLOT_PCM, n_ch * SLOTS
        views = api._view_list([dict(channel=c, n_frames=T, pcm_off=int(first[c] * SLOT_PCM), pcm_pitch=SLOT_PCM, byte_off=int(first[c] * PITCH + HEADER),
                                     byte_pitch=PITCH) for c in range(n_ch)])
        d_play = torch.from_numpy(rng.integers(-12000, 12001, ring_pcm).astype(np.int16)).cuda()  # (rooms of 8 reach the clamp, rooms of 2 do not)
        d_cap = torch.full((ring_pcm,), 77, dtype=torch.int16, device="cuda")
        d_cap_y = torch.full((ring_pcm,), 77, dtype=torch.int16, device="cuda")
        play_rows, cap_rows_y = d_play.view(ring_rows, SLOT_PCM), d_cap_y.view(ring_rows, SLOT_PCM)
        # per configuration: the ring rows of its streams' frames, [stream][t]
        rows_q = [torch.from_numpy((first[q * per:(q + 1) * per, None] + np.arange(T)[None, :]).reshape(-1)).cuda() for q in range(nq)]
        mx = pkg.Lc3Mixer(desc, 2 * n_ch)
        moved = sum(3 * per * T * nf[q] * 2 for q in range(nq))
        for room in (2, 4, 8):
            ins = np.zeros(n_ch, api.MIX_IN_DTYPE)
            ins["bus"], ins["gain_q14"] = np.arange(n_ch) // room, api.MIX_UNITY
            outs = np.zeros(n_ch, api.MIX_OUT_DTYPE)
            outs["bus"], outs["minus"] = np.arange(n_ch) // room, np.arange(n_ch)
            room_of = torch.arange(per, device="cuda") // room

            def today():
                for q in range(nq):
                    x = torch.index_select(play_rows, 0, rows_q[q])[:, :nf[q]].reshape(per, T * nf[q]).to(torch.int32)  # gather
                    tot = torch.zeros((per // room, T * nf[q]), dtype=torch.int32, device="cuda").index_add_(0, room_of, x)
                    y = (torch.index_select(tot, 0, room_of) - x).clamp_(-32768, 32767).to(torch.int16)
                    cap_rows_y[rows_q[q], :nf[q]] = y.view(per * T, nf[q])  # scatter

            def new():
                return L.lc3gpu_mix_mixed_views(mx._h, P(views), P(ins), n_ch, P(d_play), ring_pcm, P(views), P(outs), n_ch, P(d_cap), ring_pcm, P(st))

            assert new() == 0
            today()
            torch.cuda.synchronize()
            assert torch.equal(d_cap, d_cap_y), "the two routes differ"
            clamped = float(((d_cap == 32767) | (d_cap == -32768)).float().mean())
            y, w = alternate(today, new)
            my, mw = float(np.mean(y)), float(np.mean(w))
            emit(figure="mix_route", room=room, streams=n_ch, frames=T, frames_per_call=frames, clamped_share_of_ring=round(clamped, 5),
                 gather_route_ms_per_call=round(my, 4), mixer_ms_per_call=round(mw, 4), gather_route_over_mixer=round(my / mw, 3),
                 gather_route_spread=round((max(y) - min(y)) / my, 4), gather_route_rounds_ms=[round(v, 4) for v in y],
                 mixer_rounds_ms=[round(v, 4) for v in w], bytes_moved_per_call_at_least=moved, mixer_GBs=round(moved / (mw * 1e-3) / 1e9, 1),
                 measured_copy_GBs=copy_gbs, mixer_share_of_copy=round(moved / (mw * 1e-3) / 1e9 / copy_gbs, 3))
        # the whole tick, rooms of 4: what every stream sent is first made by an encoder of its own out of the playout ring's content
        room = 4
        ins = np.zeros(n_ch, api.MIX_IN_DTYPE)
        ins["bus"], ins["gain_q14"] = np.arange(n_ch) // room, api.MIX_UNITY
        outs = np.zeros(n_ch, api.MIX_OUT_DTYPE)
        outs["bus"], outs["minus"] = np.arange(n_ch) // room, np.arange(n_ch)
        ring_bytes = n_ch * SLOTS * PITCH
        d_sent = torch.zeros(ring_bytes, dtype=torch.uint8, device="cuda")
        d_back = torch.zeros(ring_bytes, dtype=torch.uint8, device="cuda")
        src = pkg.Lc3Encoder.mixed(desc)
        assert L.lc3gpu_encode_mixed_views(src._h, P(views), n_ch, P(d_play), ring_pcm, P(d_sent), ring_bytes, P(st)) == 0
        torch.cuda.synchronize()
        src.close()
        dec, enc = pkg.Lc3Decoder.mixed(desc), pkg.Lc3Encoder.mixed(desc)

        def tick(mix):
            rc = L.lc3gpu_decode_mixed_views(dec._h, P(views), n_ch, P(d_sent), ring_bytes, None, 0, P(d_play), ring_pcm, P(st))
            if mix:
                rc |= L.lc3gpu_mix_mixed_views(mx._h, P(views), P(ins), n_ch, P(d_play), ring_pcm, P(views), P(outs), n_ch, P(d_cap), ring_pcm, P(st))
            rc |= L.lc3gpu_encode_mixed_views(enc._h, P(views), n_ch, P(d_cap), ring_pcm, P(d_back), ring_bytes, P(st))
            return rc

        assert tick(True) == 0 and tick(False) == 0
        y, w = alternate(lambda: tick(False), lambda: tick(True))
        my, mw = float(np.mean(y)), float(np.mean(w))
        emit(figure="whole_tick", room=room, streams=n_ch, frames=T, frames_per_call=frames, decode_encode_ms_per_tick=round(my, 4),
             decode_mix_encode_ms_per_tick=round(mw, 4), mix_share_of_tick=round((mw - my) / mw, 4), decode_encode_spread=round((max(y) - min(y)) / my, 4),
             decode_encode_rounds_ms=[round(v, 4) for v in y], decode_mix_encode_rounds_ms=[round(v, 4) for v in w])
        dec.close(), enc.close(), mx.close()


if __name__ == "__main__":
    main()
