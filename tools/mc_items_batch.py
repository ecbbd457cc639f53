#!/usr/bin/env python3
"""The multi-channel items calls (lc3gpu_encode_mixed_mc_items / lc3gpu_decode_mixed_mc_items) against what a caller does today: the items
calls on planar buffers plus the de-interleave and multiplex copies around them.  The stream mix of profiles/r06_mixed_batch.json as
STEREO PAIRS (equal shares of the ten encodable configurations on the encoder, of all twelve on the decoder), `--frames` channel-frames
per call in two shapes -- pairs x 1 frame and a quarter of the pairs x 4 frames --, state carried, one process, one caller stream, GPU
events over `--steps` calls per measurement, the two sides alternating over `--rounds` rounds (the method of tools/mixed_list_batch.py).
One JSON line per figure, written to `--out` (default profiles/mc_items_measurements.jsonl) and printed:
  three_pass  today's route -- encode: torch de-interleave copies (one per configuration), lc3gpu_encode_mixed_items, torch multiplex
              copies; decode: the mirror -- against ONE mc call on the interleaved buffers: channel-frames/s of both, the ratio, the
              yardstick's own spread between rounds, whether both routes end in the same bytes / samples.  The yardstick's kernels are
              the parent commit's figure for figure (tests/test_mc_items_kernel_resources.py);
  kernels     the mc call against the items call ALONE (no copies), with the per-kernel milliseconds of both from lc3gpu_*_timing: what
              the strided 16-bit PCM accesses cost the front half and the synthesis, what the C * nbytes frame step costs packer and parser.
usage: python tools/mc_items_batch.py [--frames 65536] [--steps 50] [--rounds 3] [--out FILE]"""
import importlib, json, os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIXED = [(16000, 10000, 40), (24000, 10000, 60), (32000, 10000, 80), (44100, 10000, 110), (48000, 10000, 150),
         (16000, 7500, 30), (24000, 7500, 45), (32000, 7500, 60), (44100, 7500, 83), (48000, 7500, 113),
         (8000, 10000, 30), (8000, 7500, 23)]
C = 2


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    total, steps, rounds = arg("--frames", 65536), arg("--steps", 50), arg("--rounds", 3)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mc_items_measurements.jsonl")
    cmd = "python tools/mc_items_batch.py --frames %d --steps %d --rounds %d" % (total, steps, rounds)
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

    def blocks(n_cfg, pairs, T, width):
        """per configuration: (offset, elements) of its pairs' block in a buffer with `width(q)` elements per channel-frame"""
        out, off = [], 0
        for q in range(n_cfg):
            n = pairs * C * T * width(q)
            out.append((off, n))
            off += n
        return out, off

    for pairs_total, T in ((total // C, 1), (total // C // 4, 4)):
        for side in ("encode", "decode"):
            n_cfg = 10 if side == "encode" else 12
            pairs = pairs_total // n_cfg  # per configuration
            desc = [MIXED[q] for q in range(n_cfg) for _ in range(pairs * C)]
            n_ch = len(desc)
            frames = n_ch * T
            mc = np.array([(C * i, C, T, 0) for i in range(n_ch // C)], np.int32)
            flat = np.array([(c, T, 0, 0) for c in range(n_ch)], np.int32)
            pcm_blk, n_pcm = blocks(n_cfg, pairs, T, lambda q: nf[q])
            byte_blk, n_bytes = blocks(n_cfg, pairs, T, lambda q: MIXED[q][2])
            # planar PCM [channel][T][nf] per configuration, and the same audio in WAV sample order [pair][T][nf][C]
            planar = np.concatenate([np.tile(base[q][:, :T], ((pairs * C + 63) // 64, 1, 1))[:pairs * C].reshape(-1) for q in range(n_cfg)])
            d_planar_src = torch.from_numpy(planar).cuda()
            d_ilv_src = torch.empty(n_pcm, dtype=torch.int16, device="cuda")

            def views(buf, blk, q, w):  # the two layouts of configuration q's block: planar [pair][C][T][w], interleaved-by-item
                off, n = blk[q]
                return buf[off:off + n].view(pairs, C, T, w)

            def pcm_to_ilv(dst, src):  # [pair][C][T][nf] -> [pair][T][nf][C]
                for q in range(n_cfg):
                    off, n = pcm_blk[q]
                    dst[off:off + n].view(pairs, T, nf[q], C).copy_(views(src, pcm_blk, q, nf[q]).permute(0, 2, 3, 1))

            def pcm_to_planar(dst, src):
                for q in range(n_cfg):
                    off, n = pcm_blk[q]
                    views(dst, pcm_blk, q, nf[q]).copy_(src[off:off + n].view(pairs, T, nf[q], C).permute(0, 3, 1, 2))

            def bytes_to_mux(dst, src):  # [pair][C][T][nb] -> [pair][T][C][nb]
                for q in range(n_cfg):
                    off, n = byte_blk[q]
                    dst[off:off + n].view(pairs, T, C, MIXED[q][2]).copy_(views(src, byte_blk, q, MIXED[q][2]).permute(0, 2, 1, 3))

            def bytes_to_planar(dst, src):
                for q in range(n_cfg):
                    off, n = byte_blk[q]
                    views(dst, byte_blk, q, MIXED[q][2]).copy_(src[off:off + n].view(pairs, T, C, MIXED[q][2]).permute(0, 2, 1, 3))

            pcm_to_ilv(d_ilv_src, d_planar_src)
            if side == "encode":
                h_mc, h_it, h_3p = (pkg.Lc3Encoder.mixed(desc) for _ in range(3))
                L = h_mc._L
                tmp_pcm = torch.empty(n_pcm, dtype=torch.int16, device="cuda")
                tmp_out, out_3p, out_mc, out_it = (torch.zeros(n_bytes, dtype=torch.uint8, device="cuda") for _ in range(4))
                new = lambda: L.lc3gpu_encode_mixed_mc_items(h_mc._h, P(mc), len(mc), P(d_ilv_src), P(out_mc), P(st))
                alone = lambda: L.lc3gpu_encode_mixed_items(h_it._h, P(flat), n_ch, P(d_planar_src), P(out_it), P(st))

                def today():
                    pcm_to_planar(tmp_pcm, d_ilv_src)
                    L.lc3gpu_encode_mixed_items(h_3p._h, P(flat), n_ch, P(tmp_pcm), P(tmp_out), P(st))
                    bytes_to_mux(out_3p, tmp_out)
            else:
                src = pkg.Lc3Encoder.mixed(desc, spec_flags=api.SPEC_8KHZ_ENCODE)
                d_in_planar = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
                src.encode_mixed_items([tuple(r[:3]) for r in flat.tolist()], d_planar_src, d_in_planar, stream=st)
                d_in_mux = torch.empty_like(d_in_planar)
                bytes_to_mux(d_in_mux, d_in_planar)
                torch.cuda.synchronize()
                del src
                h_mc, h_it, h_3p = (pkg.Lc3Decoder.mixed(desc) for _ in range(3))
                L = h_mc._L
                tmp_in = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
                tmp_out, out_3p, out_mc, out_it = (torch.zeros(n_pcm, dtype=torch.int16, device="cuda") for _ in range(4))
                new = lambda: L.lc3gpu_decode_mixed_mc_items(h_mc._h, P(mc), len(mc), P(d_in_mux), None, P(out_mc), P(st))
                alone = lambda: L.lc3gpu_decode_mixed_items(h_it._h, P(flat), n_ch, P(d_in_planar), None, P(out_it), P(st))

                def today():
                    bytes_to_planar(tmp_in, d_in_mux)
                    L.lc3gpu_decode_mixed_items(h_3p._h, P(flat), n_ch, P(tmp_in), None, P(tmp_out), P(st))
                    pcm_to_ilv(out_3p, tmp_out)
            today(), new(), alone()
            torch.cuda.synchronize()
            same = bool(torch.equal(out_3p, out_mc))
            y, w = alternate(today, new, frames)
            my, mw = float(np.mean(y)), float(np.mean(w))
            emit(figure="three_pass", side=side, pairs=n_ch // C, frames=T, channel_frames=frames, copies_per_pass=n_cfg,
                 today_frames_per_s=round(my), mc_frames_per_s=round(mw), mc_over_today=round(mw / my, 4), today_spread=round((max(y) - min(y)) / my, 4),
                 today_rounds=[round(x) for x in y], mc_rounds=[round(x) for x in w], same_output=same)
            y, w = alternate(alone, new, frames)
            my, mw = float(np.mean(y)), float(np.mean(w))
            emit(figure="kernels", side=side, pairs=n_ch // C, frames=T, channel_frames=frames, items_alone_frames_per_s=round(my), mc_frames_per_s=round(mw),
                 mc_over_items_alone=round(mw / my, 4), items_spread=round((max(y) - min(y)) / my, 4), items_kernel_ms_per_call=kernel_ms(h_it, alone),
                 mc_kernel_ms_per_call=kernel_ms(h_mc, new))
            del h_mc, h_it, h_3p


if __name__ == "__main__":
    main()
