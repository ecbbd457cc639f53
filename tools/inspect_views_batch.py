#!/usr/bin/env python3
"""lc3gpu_inspect_mixed_views against what a caller does today for the per-frame status of a tick in rings: a torch gather of frames and
flags per (configuration, size), one lc3gpu_inspect per bucket, a scatter of the statuses (and of the records) back to the rings'
placement.  The stream mix of profiles/r06_mixed_batch.json (equal shares of all twelve configurations), `--frames` frames per call in
two shapes -- streams x 1 frame and a quarter of the streams x 4 frames --, rings as in tools/views_batch.py (8 slots of 400 bytes behind
a 12-byte header, 8 flags per stream), one process, one caller stream, GPU events over `--steps` calls per measurement, the two routes
alternating over `--rounds` rounds.  One JSON line per figure, written to `--out` (default profiles/inspect_views_measurements.jsonl) and
printed:
  gather_route  today's route against ONE inspector call on the rings, status only and with records: frames/s of both, the ratio, the
                yardstick's own spread between rounds, whether both routes leave identical arrays.  The yardstick's kernel is the main
                library's lc3_inspect_kernel, untouched;
  kernel_alone  the inspector call on COMPACT placements against the twelve lc3gpu_inspect calls alone on the same frames compact (no
                copies): what finding the frames through the rows and copying them lane by lane cost.
usage: python tools/inspect_views_batch.py [--frames 65536] [--steps 50] [--rounds 3] [--out FILE]"""
import importlib, json, os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIXED = [(16000, 10000, 40), (24000, 10000, 60), (32000, 10000, 80), (44100, 10000, 110), (48000, 10000, 150),
         (16000, 7500, 30), (24000, 7500, 45), (32000, 7500, 60), (44100, 7500, 83), (48000, 7500, 113),
         (8000, 10000, 30), (8000, 7500, 23)]
SLOTS, HEADER, SLOT_BYTES = 8, 12, 400
PITCH = HEADER + SLOT_BYTES


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    total, steps, rounds = arg("--frames", 65536), arg("--steps", 50), arg("--rounds", 3)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "inspect_views_measurements.jsonl")
    cmd = "python tools/inspect_views_batch.py --frames %d --steps %d --rounds %d" % (total, steps, rounds)
    open(out_path, "w").close()  # a run replaces the file
    import torch

    pkg = importlib.import_module("lc3-codec_amd")
    api = importlib.import_module("lc3-codec_amd.api")
    synth = importlib.import_module("lc3-codec_amd.synth")
    st = torch.cuda.current_stream().cuda_stream
    nf = [pkg.Lc3Config(fs, us).nf for fs, us, _ in MIXED]
    base = [synth.make_pcm(64, 4, nf[k], MIXED[k][0], seed=51) for k in range(12)]
    P = api._ptr
    L = pkg.load_library()

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

    for streams_total, T in ((total, 1), (total // 4, 4)):
        per = streams_total // 12
        cfg_of = [q for q in range(12) for _ in range(per)]
        desc = [MIXED[q] for q in cfg_of]
        n_ch = len(desc)
        frames = n_ch * T
        rng = np.random.default_rng(5)
        slot0 = rng.integers(0, SLOTS - T + 1, n_ch)
        widths_b = np.array([MIXED[q][2] for q in cfg_of])
        bo = np.concatenate([[0], np.cumsum(T * widths_b)])
        n_bytes = int(bo[-1])
        # the tick's frames: encoded compact in stream order, one frame in twelve damaged, one in a hundred flagged; then put into the rings
        planar = np.concatenate([np.tile(base[q][:, :T], ((per + 63) // 64, 1, 1))[:per].reshape(-1) for q in range(12)])
        src = pkg.Lc3Encoder.mixed(desc, spec_flags=api.SPEC_8KHZ_ENCODE)
        d_compact = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
        src.encode_mixed_items([(c, T, 0) for c in range(n_ch)], torch.from_numpy(planar).cuda(), d_compact, stream=st)
        torch.cuda.synchronize()
        del src
        hit = torch.from_numpy(rng.integers(0, n_bytes, frames // 12)).cuda()
        d_compact[hit] ^= 0x10
        ring_bytes, ring_flags = n_ch * SLOTS * PITCH, n_ch * SLOTS
        first = np.arange(n_ch) * SLOTS + slot0  # first ring slot of every stream's frames
        views_ring = api._view_list([dict(channel=c, n_frames=T, pcm_off=0, byte_off=int(first[c] * PITCH + HEADER), byte_pitch=PITCH,
                                          flag_off=int(first[c]), flag_pitch=1) for c in range(n_ch)])
        views_compact = api._view_list([dict(channel=c, n_frames=T, pcm_off=0, byte_off=int(bo[c]), flag_off=c * T) for c in range(n_ch)])
        # per bucket (= configuration: one size each in this mix): element indices of its frames in the rings and in the compact buffer
        buckets = []
        for q in range(12):
            ch = np.arange(q * per, (q + 1) * per)
            nb = MIXED[q][2]
            slots = (first[ch][:, None] + np.arange(T)[None, :]).reshape(-1)  # [stream][t]
            idx_ring = (slots[:, None] * PITCH + HEADER + np.arange(nb)[None, :]).reshape(-1)
            n = len(slots)
            buckets.append(dict(q=q, n=n, nb=nb, idx_bytes=torch.from_numpy(idx_ring).cuda(), idx_flags=torch.from_numpy(slots).cuda(),
                                compact_at=int(bo[q * per]), tmp_in=torch.empty(n * nb, dtype=torch.uint8, device="cuda"),
                                tmp_fl=torch.empty(n, dtype=torch.uint8, device="cuda"), rec=torch.zeros((n, 32), dtype=torch.int32, device="cuda"),
                                rec_alone=torch.zeros((n, 32), dtype=torch.int32, device="cuda")))
        d_ring_in = torch.zeros(ring_bytes, dtype=torch.uint8, device="cuda")
        for b in buckets:
            d_ring_in[b["idx_bytes"]] = d_compact[b["compact_at"]: b["compact_at"] + b["n"] * b["nb"]]
        d_ring_flags = torch.from_numpy((rng.random(ring_flags) < 0.01).astype(np.uint8)).cuda()
        d_flags_compact = torch.cat([d_ring_flags[b["idx_flags"]] for b in buckets])
        insp = pkg.Lc3Inspector(desc, n_ch)
        st_vw, st_gr, st_cv = (torch.full((ring_flags,), 0xCC, dtype=torch.uint8, device="cuda") for _ in range(3))
        in_vw, in_gr = (torch.full((ring_flags, 32), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        in_cv = torch.full((frames, 32), -7, dtype=torch.int32, device="cuda")
        call = lambda v, d_in, n_in, fl, n_fl, s, n_s, i, n_i: L.lc3gpu_inspect_mixed_views(insp._h, P(v), n_ch, P(d_in), n_in, P(fl), n_fl, P(s), n_s, P(i), n_i, P(st))
        new_status = lambda: call(views_ring, d_ring_in, ring_bytes, d_ring_flags, ring_flags, st_vw, ring_flags, None, 0)
        new_records = lambda: call(views_ring, d_ring_in, ring_bytes, d_ring_flags, ring_flags, st_vw, ring_flags, in_vw, ring_flags)
        new_compact = lambda: call(views_compact, d_compact, n_bytes, d_flags_compact, frames, st_cv, frames, in_cv, frames)

        def today(records):
            for b in buckets:
                fs, us, nb = MIXED[b["q"]]
                torch.index_select(d_ring_in, 0, b["idx_bytes"], out=b["tmp_in"])
                torch.index_select(d_ring_flags, 0, b["idx_flags"], out=b["tmp_fl"])
                L.lc3gpu_inspect(us, fs, P(b["tmp_in"]), None, P(b["tmp_fl"]), nb, b["n"], P(b["rec"]), P(st))
                st_gr.index_copy_(0, b["idx_flags"], b["rec"][:, 0].to(torch.uint8))
                if records:
                    in_gr.index_copy_(0, b["idx_flags"], b["rec"])

        def alone():
            at = 0
            for b in buckets:
                fs, us, nb = MIXED[b["q"]]
                L.lc3gpu_inspect(us, fs, d_compact.data_ptr() + b["compact_at"], None, d_flags_compact.data_ptr() + at, nb, b["n"], P(b["rec_alone"]), P(st))
                at += b["n"]

        rcs = (new_records(), new_compact())
        today(True)
        alone()
        torch.cuda.synchronize()
        assert rcs == (0, 0), rcs
        same = bool(torch.equal(st_vw, st_gr) and torch.equal(in_vw, in_gr))
        same_compact = bool(torch.equal(in_cv, torch.cat([b["rec_alone"] for b in buckets])) and torch.equal(st_cv[:frames], in_cv[:, 0].to(torch.uint8)))
        lost = float((in_cv[:, 0] != 0).float().mean())
        for form, new in (("status", new_status), ("records", new_records)):
            y, w = alternate(lambda: today(form == "records"), new, frames)
            my, mw = float(np.mean(y)), float(np.mean(w))
            emit(figure="gather_route", form=form, streams=n_ch, frames=T, frames_per_call=frames, status_nonzero_share=round(lost, 4),
                 gather_frames_per_s=round(my), inspector_frames_per_s=round(mw), inspector_over_gather=round(mw / my, 4),
                 gather_spread=round((max(y) - min(y)) / my, 4), gather_rounds=[round(x) for x in y], inspector_rounds=[round(x) for x in w],
                 same_output=same)
        y, w = alternate(alone, new_compact, frames)
        my, mw = float(np.mean(y)), float(np.mean(w))
        emit(figure="kernel_alone", streams=n_ch, frames=T, frames_per_call=frames, inspect_x12_ms_per_call=round(frames / my * 1e3, 4),
             inspector_ms_per_call=round(frames / mw * 1e3, 4), inspector_over_inspect_x12=round(mw / my, 4), inspect_spread=round((max(y) - min(y)) / my, 4),
             same_output=same_compact)
        insp.close()


if __name__ == "__main__":
    main()
