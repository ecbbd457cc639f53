#!/usr/bin/env python3
"""The views calls (lc3gpu_encode_mixed_views / lc3gpu_decode_mixed_views) against what a caller does today: the items calls on compact
buffers plus the gather and scatter passes around them.  The stream mix of profiles/r06_mixed_batch.json (equal shares of the ten
encodable configurations on the encoder, of all twelve on the decoder), `--frames` frames per call in two shapes -- streams x 1 frame and
a quarter of the streams x 4 frames --, state carried, one process, one caller stream, GPU events over `--steps` calls per measurement,
the two sides alternating over `--rounds` rounds (the method of tools/mc_items_batch.py).  Every stream owns rings as a server keeps
them: 8 byte slots of 400 bytes behind a 12-byte header (pitch 412), 8 PCM slots of 480 samples, 8 flags; a call's frames of a stream
start at slot 0 .. 4.  One JSON line per figure, written to `--out` (default profiles/views_measurements.jsonl) and printed:
  gather_route  today's route -- decode: torch index-gather of frames and flags out of the rings, lc3gpu_decode_mixed_items, torch
                index-scatter of the PCM into the rings; encode: the mirror -- against ONE views call on the rings: frames/s of both, the
                ratio, the yardstick's own spread between rounds, whether both routes end in identical bytes / samples.  The yardstick's
                kernels are the parent commit's figure for figure (tests/test_views_kernel_resources.py);
  kernels       the views call on COMPACT placements against the items call ALONE (no copies), with the per-kernel milliseconds of both
                from lc3gpu_*_timing: what the row loads and the pitch arithmetic cost.
usage: python tools/views_batch.py [--frames 65536] [--steps 50] [--rounds 3] [--out FILE]"""
import importlib, json, os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIXED = [(16000, 10000, 40), (24000, 10000, 60), (32000, 10000, 80), (44100, 10000, 110), (48000, 10000, 150),
         (16000, 7500, 30), (24000, 7500, 45), (32000, 7500, 60), (44100, 7500, 83), (48000, 7500, 113),
         (8000, 10000, 30), (8000, 7500, 23)]
SLOTS, HEADER, SLOT_BYTES, SLOT_PCM = 8, 12, 400, 480
PITCH = HEADER + SLOT_BYTES


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    total, steps, rounds = arg("--frames", 65536), arg("--steps", 50), arg("--rounds", 3)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "views_measurements.jsonl")
    cmd = "python tools/views_batch.py --frames %d --steps %d --rounds %d" % (total, steps, rounds)
    open(out_path, "w").close()  # a run replaces the file: measured rows never sit beside rows of an earlier run or "not measured" ones
    import torch

    pkg = importlib.import_module("lc3-codec_amd")
    api = importlib.import_module("lc3-codec_amd.api")
    synth = importlib.import_module("lc3-codec_amd.synth")
    st = torch.cuda.current_stream().cuda_stream
    nf = [pkg.Lc3Config(fs, us).nf for fs, us, _ in MIXED]
    base = [synth.make_pcm(64, 4, nf[k], MIXED[k][0], seed=51) for k in range(12)]
    P = api._ptr

    def emit(**row):
        row["command"] = cmd
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")

    def events(call, frames_per_call):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            call()
        b.record()
        torch.cuda.synchronize()
        return frames_per_call * steps / (a.elapsed_time(b) * 1e-3)

    def alternate(yard, new, frames_per_call):
        for _ in range(3):
            yard()
            new()
        y, n = [], []
        for _ in range(rounds):
            y.append(events(yard, frames_per_call))
            n.append(events(new, frames_per_call))
        return y, n

    def kernel_ms(h, call):
        h.timing(True)
        for _ in range(10):
            call()
        return [round(x / 10, 4) for x in h.timing(False)[:-1]]

    for streams_total, T in ((total, 1), (total // 4, 4)):
        for side in ("encode", "decode"):
            n_cfg = 10 if side == "encode" else 12
            per = streams_total // n_cfg
            cfg_of = [q for q in range(n_cfg) for _ in range(per)]
            desc = [MIXED[q] for q in cfg_of]
            n_ch = len(desc)
            frames = n_ch * T
            rng = np.random.default_rng(5)
            slot0 = rng.integers(0, SLOTS - T + 1, n_ch)
            items = np.array([(c, T, 0, 0) for c in range(n_ch)], np.int32)
            # compact placements (the items call's prefix sums) and the rings', as views and as element indices for torch
            widths_p, widths_b = np.array([nf[q] for q in cfg_of]), np.array([MIXED[q][2] for q in cfg_of])
            po = np.concatenate([[0], np.cumsum(T * widths_p)])
            bo = np.concatenate([[0], np.cumsum(T * widths_b)])
            n_pcm, n_bytes = int(po[-1]), int(bo[-1])
            compact = api._view_list([dict(channel=c, n_frames=T, pcm_off=int(po[c]), byte_off=int(bo[c]), flag_off=c * T) for c in range(n_ch)])
            ring = api._view_list([dict(channel=c, n_frames=T, pcm_off=int((c * SLOTS + slot0[c]) * SLOT_PCM), pcm_pitch=SLOT_PCM,
                                        byte_off=int((c * SLOTS + slot0[c]) * PITCH + HEADER), byte_pitch=PITCH, flag_off=int(c * SLOTS + slot0[c]),
                                        flag_pitch=1) for c in range(n_ch)])
            ring_pcm, ring_bytes, ring_flags = n_ch * SLOTS * SLOT_PCM, n_ch * SLOTS * PITCH, n_ch * SLOTS

            def index(width, slot_elems, first):  # element index in the rings of every element of the compact buffer, in its order
                out = []
                for c in range(n_ch):
                    fr = (c * SLOTS + slot0[c] + np.arange(T))[:, None] * slot_elems + first + np.arange(width[c])[None, :]
                    out.append(fr.reshape(-1))
                return torch.from_numpy(np.concatenate(out)).cuda()

            idx_pcm, idx_bytes = index(widths_p, SLOT_PCM, 0), index(widths_b, PITCH, HEADER)
            idx_flags = torch.from_numpy(np.concatenate([c * SLOTS + slot0[c] + np.arange(T) for c in range(n_ch)])).cuda()
            planar = np.concatenate([np.tile(base[q][:, :T], ((per + 63) // 64, 1, 1))[:per].reshape(-1) for q in range(n_cfg)])
            d_compact_pcm = torch.from_numpy(planar).cuda()
            d_ring_pcm = torch.zeros(ring_pcm, dtype=torch.int16, device="cuda")
            d_ring_pcm[idx_pcm] = d_compact_pcm
            d_ring_flags = torch.zeros(ring_flags, dtype=torch.uint8, device="cuda")
            if side == "encode":
                h_vw, h_it, h_gr, h_cv = (pkg.Lc3Encoder.mixed(desc) for _ in range(4))
                L = h_vw._L
                tmp_pcm = torch.empty(n_pcm, dtype=torch.int16, device="cuda")
                tmp_out, out_it, out_cv = (torch.zeros(n_bytes, dtype=torch.uint8, device="cuda") for _ in range(3))
                ring_vw, ring_gr = (torch.zeros(ring_bytes, dtype=torch.uint8, device="cuda") for _ in range(2))
                new = lambda: L.lc3gpu_encode_mixed_views(h_vw._h, P(ring), n_ch, P(d_ring_pcm), ring_pcm, P(ring_vw), ring_bytes, P(st))
                alone = lambda: L.lc3gpu_encode_mixed_items(h_it._h, P(items), n_ch, P(d_compact_pcm), P(out_it), P(st))
                new_compact = lambda: L.lc3gpu_encode_mixed_views(h_cv._h, P(compact), n_ch, P(d_compact_pcm), n_pcm, P(out_cv), n_bytes, P(st))

                def today():
                    torch.index_select(d_ring_pcm, 0, idx_pcm, out=tmp_pcm)
                    L.lc3gpu_encode_mixed_items(h_gr._h, P(items), n_ch, P(tmp_pcm), P(tmp_out), P(st))
                    ring_gr.index_copy_(0, idx_bytes, tmp_out)
            else:
                src = pkg.Lc3Encoder.mixed(desc, spec_flags=api.SPEC_8KHZ_ENCODE)
                d_in_compact = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
                src.encode_mixed_items([tuple(r[:3]) for r in items.tolist()], d_compact_pcm, d_in_compact, stream=st)
                d_ring_in = torch.zeros(ring_bytes, dtype=torch.uint8, device="cuda")
                d_ring_in[idx_bytes] = d_in_compact
                d_flags_compact = torch.zeros(frames, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                del src
                h_vw, h_it, h_gr, h_cv = (pkg.Lc3Decoder.mixed(desc) for _ in range(4))
                L = h_vw._L
                tmp_in = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
                tmp_fl = torch.empty(frames, dtype=torch.uint8, device="cuda")
                tmp_out, out_it, out_cv = (torch.zeros(n_pcm, dtype=torch.int16, device="cuda") for _ in range(3))
                ring_vw, ring_gr = (torch.zeros(ring_pcm, dtype=torch.int16, device="cuda") for _ in range(2))
                new = lambda: L.lc3gpu_decode_mixed_views(h_vw._h, P(ring), n_ch, P(d_ring_in), ring_bytes, P(d_ring_flags), ring_flags, P(ring_vw),
                                                          ring_pcm, P(st))
                alone = lambda: L.lc3gpu_decode_mixed_items(h_it._h, P(items), n_ch, P(d_in_compact), P(d_flags_compact), P(out_it), P(st))
                new_compact = lambda: L.lc3gpu_decode_mixed_views(h_cv._h, P(compact), n_ch, P(d_in_compact), n_bytes, P(d_flags_compact), frames,
                                                                  P(out_cv), n_pcm, P(st))

                def today():
                    torch.index_select(d_ring_in, 0, idx_bytes, out=tmp_in)
                    torch.index_select(d_ring_flags, 0, idx_flags, out=tmp_fl)
                    L.lc3gpu_decode_mixed_items(h_gr._h, P(items), n_ch, P(tmp_in), P(tmp_fl), P(tmp_out), P(st))
                    ring_gr.index_copy_(0, idx_pcm, tmp_out)
            rcs = (new(), alone(), new_compact())
            today()
            torch.cuda.synchronize()
            assert rcs == (0, 0, 0), rcs
            same = bool(torch.equal(ring_gr, ring_vw))
            same_compact = bool(torch.equal(out_it, out_cv))
            y, w = alternate(today, new, frames)
            my, mw = float(np.mean(y)), float(np.mean(w))
            emit(figure="gather_route", side=side, streams=n_ch, frames=T, frames_per_call=frames, gather_frames_per_s=round(my), views_frames_per_s=round(mw),
                 views_over_gather=round(mw / my, 4), gather_spread=round((max(y) - min(y)) / my, 4), gather_rounds=[round(x) for x in y],
                 views_rounds=[round(x) for x in w], same_output=same)
            y, w = alternate(alone, new_compact, frames)
            my, mw = float(np.mean(y)), float(np.mean(w))
            emit(figure="kernels", side=side, streams=n_ch, frames=T, frames_per_call=frames, items_alone_frames_per_s=round(my), views_frames_per_s=round(mw),
                 views_over_items_alone=round(mw / my, 4), items_spread=round((max(y) - min(y)) / my, 4), same_output=same_compact,
                 items_kernel_ms_per_call=kernel_ms(h_it, alone), views_kernel_ms_per_call=kernel_ms(h_cv, new_compact))
            del h_vw, h_it, h_gr, h_cv


if __name__ == "__main__":
    main()
