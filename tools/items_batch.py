#!/usr/bin/env python3
"""The items calls (lc3gpu_encode_mixed_items / lc3gpu_decode_mixed_items) against the mixed-list calls on the same handle shape: the
stream mix of profiles/r06_mixed_batch.json (equal shares of the ten encodable configurations on the encoder, of all twelve on the
decoder), state carried, one process, one caller stream, GPU events over `--steps` calls per measurement, the two sides of every
comparison alternating over `--rounds` rounds (the method of tools/mixed_list_batch.py).  One JSON line per figure, appended to `--out`
(default profiles/items_measurements.jsonl) and printed:
  degenerate  items with one common T and the descriptors' sizes (every channel, in order) against lc3gpu_*_mixed_list at `--streams` x 1
              and `--streams`/4 x 4: frames/s of both sides, their ratio, the spread between the repeated mixed-list measurements,
              whether the ratio holds 0.952 less that spread, and the per-kernel times of both sides when it does not.  The yardstick is
              the mixed-list call of THIS library: its kernels are the parent commit's figure for figure
              (tests/test_items_kernel_resources.py::test_no_kernel_of_the_parent_changed) and its host path is the parent's;
  host        wall time of one call that does not wait for the device (checks + plan + upload + launches) at `--streams` items, beside the
              mixed-list call's;
  tick_30_ms  four frames of every 7.5 ms stream and three of every 10 ms stream as ONE items call against today's alternative, two
              mixed-list calls split by duration: microseconds per tick and frames/s of both.
usage: python tools/items_batch.py [--streams 65536] [--steps 50] [--rounds 3] [--out FILE]"""
import importlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ALLOWANCE = 0.952  # DESIGN section 3, channel lists: what the list calls were held to over their yardsticks
MIXED = [(16000, 10000, 40), (24000, 10000, 60), (32000, 10000, 80), (44100, 10000, 110), (48000, 10000, 150),
         (16000, 7500, 30), (24000, 7500, 45), (32000, 7500, 60), (44100, 7500, 83), (48000, 7500, 113),
         (8000, 10000, 30), (8000, 7500, 23)]


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    total, steps, rounds = arg("--streams", 65536), arg("--steps", 50), arg("--rounds", 3)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "items_measurements.jsonl")
    cmd = "python tools/items_batch.py --streams %d --steps %d --rounds %d" % (total, steps, rounds)
    import torch

    pkg = importlib.import_module("lc3-codec_amd")
    api = importlib.import_module("lc3-codec_amd.api")
    synth = importlib.import_module("lc3-codec_amd.synth")
    st = torch.cuda.current_stream().cuda_stream
    nf = [pkg.Lc3Config(fs, us).nf for fs, us, _ in MIXED]
    base = [synth.make_pcm(64, 4, nf[k], MIXED[k][0], seed=51) for k in range(12)]

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

    def host_us(call, n=20):
        t = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        return round(float(np.median(t)), 1)

    def setup(N, T):
        """descriptors, the encoder's PCM and the decoder's input for T frames of N streams, stream-major ragged"""
        Se, Sd = N // 10, N // 12
        enc_desc = [MIXED[q] for q in range(10) for _ in range(Se)]
        dec_desc = [MIXED[q] for q in range(12) for _ in range(Sd)]
        tile = lambda q, S: np.tile(base[q][:, :T], ((S + 63) // 64, 1, 1))[:S].reshape(-1)
        d_pcm = torch.from_numpy(np.concatenate([tile(q, Se) for q in range(10)])).cuda()
        src = pkg.Lc3Encoder.mixed(dec_desc, spec_flags=api.SPEC_8KHZ_ENCODE)
        d_in = torch.zeros(sum(T * d[2] for d in dec_desc), dtype=torch.uint8, device="cuda")
        src.encode_mixed(torch.from_numpy(np.concatenate([tile(q, Sd) for q in range(12)])).cuda(), d_in, T, stream=st)
        torch.cuda.synchronize()
        return Se, Sd, enc_desc, dec_desc, d_pcm, d_in

    for N, T in ((total, 1), (total // 4, 4)):
        Se, Sd, enc_desc, dec_desc, d_pcm, d_in = setup(N, T)
        ne, nd = len(enc_desc), len(dec_desc)
        enc_l, enc_i = pkg.Lc3Encoder.mixed(enc_desc), pkg.Lc3Encoder.mixed(enc_desc)
        dec_l, dec_i = pkg.Lc3Decoder.mixed(dec_desc), pkg.Lc3Decoder.mixed(dec_desc)
        b_l, b_i = (torch.zeros(sum(T * d[2] for d in enc_desc), dtype=torch.uint8, device="cuda") for _ in range(2))
        p_l, p_i = (torch.zeros(sum(T * nf[q] * Sd for q in range(12)), dtype=torch.int16, device="cuda") for _ in range(2))
        che, chd = np.arange(ne, dtype=np.int32), np.arange(nd, dtype=np.int32)
        ite = np.zeros((ne, 4), np.int32)
        ite[:, 0], ite[:, 1] = che, T
        itd = np.zeros((nd, 4), np.int32)
        itd[:, 0], itd[:, 1] = chd, T
        P, L = api._ptr, enc_i._L  # (the items arrays are built once, as the channel lists are: the calls are timed, not numpy)
        e_l = lambda: enc_l.encode_mixed_list(che, d_pcm, b_l, T, stream=st)
        e_i = lambda: L.lc3gpu_encode_mixed_items(enc_i._h, P(ite), ne, P(d_pcm), P(b_i), P(st))
        d_l = lambda: dec_l.decode_mixed_list(chd, d_in, p_l, T, stream=st)
        d_i = lambda: L.lc3gpu_decode_mixed_items(dec_i._h, P(itd), nd, P(d_in), None, P(p_i), P(st))
        e_l(), e_i(), d_l(), d_i()
        torch.cuda.synchronize()
        same = {"encode": bool(torch.equal(b_l, b_i)), "decode": bool(torch.equal(p_l, p_i))}
        for side, fy, fn, hy, hn, n in (("encode", e_l, e_i, enc_l, enc_i, ne), ("decode", d_l, d_i, dec_l, dec_i, nd)):
            y, w = alternate(fy, fn, n * T)
            my, mw = float(np.mean(y)), float(np.mean(w))
            spread = (max(y) - min(y)) / my
            row = {"figure": "degenerate", "side": side, "streams": n, "frames": T, "mixed_list_frames_per_s": round(my), "items_frames_per_s": round(mw),
                   "items_over_mixed_list": round(mw / my, 4), "mixed_list_spread": round(spread, 4), "mixed_list_rounds": [round(x) for x in y],
                   "items_rounds": [round(x) for x in w], "same_output": same[side], "allowance": ALLOWANCE,
                   "holds_allowance": bool(mw / my >= ALLOWANCE - spread)}
            if not row["holds_allowance"]:
                for name, h, f in (("mixed_list", hy, fy), ("items", hn, fn)):
                    h.timing(True)
                    for _ in range(10):
                        f()
                    row[name + "_kernel_ms_per_call"] = [round(x / 10, 4) for x in h.timing(False)[:-1]]
            emit(**row)
        if T == 1:
            emit(figure="host_us_per_call", n_items_encode=ne, n_items_decode=nd, upload_bytes_per_item=28, encode_mixed_list=host_us(e_l),
                 encode_mixed_items=host_us(e_i), decode_mixed_list=host_us(d_l), decode_mixed_items=host_us(d_i))
        del enc_l, enc_i, dec_l, dec_i

    # the 30 ms tick: four frames of the 7.5 ms streams, three of the 10 ms streams
    N = total // 4
    owed = lambda d: 4 if d[1] == 7500 else 3
    for side in ("encode", "decode"):
        n_cfg = 10 if side == "encode" else 12
        S = N // n_cfg
        desc = [MIXED[q] for q in range(n_cfg) for _ in range(S)]
        n = len(desc)
        tile = lambda q, T: np.tile(base[q][:, :T], ((S + 63) // 64, 1, 1))[:S].reshape(-1)
        pcm_items = torch.from_numpy(np.concatenate([tile(q, owed(MIXED[q])) for q in range(n_cfg)])).cuda()
        parts = {us: [c for c in range(n) if desc[c][1] == us] for us in (7500, 10000)}
        cfgs = {us: [q for q in range(n_cfg) if MIXED[q][1] == us] for us in (7500, 10000)}
        pcm_part = {us: torch.from_numpy(np.concatenate([tile(q, owed(MIXED[q])) for q in cfgs[us]])).cuda() for us in (7500, 10000)}
        nbytes_of = lambda cs: sum(owed(desc[c]) * desc[c][2] for c in cs)
        npcm_of = lambda cs: sum(owed(desc[c]) * nf[MIXED.index(desc[c])] for c in cs)
        it = np.array([(c, owed(desc[c]), 0, 0) for c in range(n)], np.int32)
        lists = {us: np.array(parts[us], np.int32) for us in parts}
        frames = sum(owed(d) for d in desc)
        P = api._ptr
        if side == "encode":
            h_i, h_l = pkg.Lc3Encoder.mixed(desc), pkg.Lc3Encoder.mixed(desc)
            out_i = torch.zeros(nbytes_of(range(n)), dtype=torch.uint8, device="cuda")
            out_p = {us: torch.zeros(nbytes_of(parts[us]), dtype=torch.uint8, device="cuda") for us in parts}
            one = lambda: h_i._L.lc3gpu_encode_mixed_items(h_i._h, P(it), n, P(pcm_items), P(out_i), P(st))

            def two():
                for us in (7500, 10000):
                    h_l.encode_mixed_list(lists[us], pcm_part[us], out_p[us], owed((0, us)), stream=st)
        else:
            src = pkg.Lc3Encoder.mixed(desc, spec_flags=api.SPEC_8KHZ_ENCODE)
            in_i = torch.zeros(nbytes_of(range(n)), dtype=torch.uint8, device="cuda")
            src.encode_mixed_items([tuple(r[:3]) for r in it.tolist()], pcm_items, in_i, stream=st)
            in_p = {us: torch.zeros(nbytes_of(parts[us]), dtype=torch.uint8, device="cuda") for us in parts}
            for us in parts:
                src.reset()
                src.encode_mixed_list(lists[us], pcm_part[us], in_p[us], owed((0, us)), stream=st)
            torch.cuda.synchronize()
            del src
            h_i, h_l = pkg.Lc3Decoder.mixed(desc), pkg.Lc3Decoder.mixed(desc)
            out_i = torch.zeros(npcm_of(range(n)), dtype=torch.int16, device="cuda")
            out_p = {us: torch.zeros(npcm_of(parts[us]), dtype=torch.int16, device="cuda") for us in parts}
            one = lambda: h_i._L.lc3gpu_decode_mixed_items(h_i._h, P(it), n, P(in_i), None, P(out_i), P(st))

            def two():
                for us in (7500, 10000):
                    h_l.decode_mixed_list(lists[us], in_p[us], out_p[us], owed((0, us)), stream=st)
        y, w = alternate(two, one, frames)
        my, mw = float(np.mean(y)), float(np.mean(w))
        emit(figure="tick_30_ms", side=side, streams=n, frames_per_tick=frames, two_mixed_list_calls_frames_per_s=round(my), one_items_call_frames_per_s=round(mw),
             two_mixed_list_calls_us_per_tick=round(frames / my * 1e6, 1), one_items_call_us_per_tick=round(frames / mw * 1e6, 1),
             items_over_two_calls=round(mw / my, 4), two_calls_rounds=[round(x) for x in y], items_rounds=[round(x) for x in w],
             two_calls_host_us=host_us(two), items_host_us=host_us(one))
        del h_i, h_l


if __name__ == "__main__":
    main()
