#!/usr/bin/env python3
"""The mixed-list calls (lc3gpu_encode_mixed_list / lc3gpu_decode_mixed_list) against lc3gpu_encode_mixed / lc3gpu_decode_mixed on the same
handle shape: the stream mix of profiles/r06_mixed_batch.json (equal shares of the ten encodable configurations on the encoder, of all
twelve on the decoder, configuration by configuration), state carried, one process, one caller stream, GPU events over `--steps` calls per
measurement, the two sides of every comparison alternating (the method of tools/list_batch.py).  One JSON line per figure:
  parity     list = 0 .. n-1 against the mixed call at `--streams` x 1 and `--streams`/4 x 4: frames/s of both sides (mean of `--rounds`
             alternating measurements), their ratio, the spread between the repeated mixed-call measurements, whether the ratio holds
             0.952 (what the uniform list calls were held to) less that spread, and the per-kernel times of both sides when it does not;
  host       wall time of one call that does not wait for the device (checks + plan + upload + launches) at n_list = `--streams`, beside
             the same for the mixed call (median over calls with an idle device);
  subset     a random half and a random eighth of the channels per tick, one frame, 1 % of the listed channels reset before the tick;
  clock      the ticks of a 2.5 ms clock (7.5 ms streams due every third step, 10 ms streams every fourth, a due stream dropped with
             probability 0.2), the twelve steps of one period taking turns: frames/s and microseconds per tick.
usage: python tools/mixed_list_batch.py [--streams 65536] [--steps 50] [--rounds 3]"""
import importlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ALLOWANCE = 0.952  # DESIGN section 3, channel lists: the list calls over their uniform twins, as accepted
MIXED = [(16000, 10000, 40), (24000, 10000, 60), (32000, 10000, 80), (44100, 10000, 110), (48000, 10000, 150),
         (16000, 7500, 30), (24000, 7500, 45), (32000, 7500, 60), (44100, 7500, 83), (48000, 7500, 113),
         (8000, 10000, 30), (8000, 7500, 23)]


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    total, steps, rounds = arg("--streams", 65536), arg("--steps", 50), arg("--rounds", 3)
    cmd = "python tools/mixed_list_batch.py --streams %d --steps %d --rounds %d" % (total, steps, rounds)
    import torch

    pkg = importlib.import_module("lc3-codec_amd")
    synth = importlib.import_module("lc3-codec_amd.synth")
    st = torch.cuda.current_stream().cuda_stream
    nf = [pkg.Lc3Config(fs, us).nf for fs, us, _ in MIXED]
    base = [synth.make_pcm(64, 4, nf[k], MIXED[k][0], seed=51) for k in range(12)]

    def emit(**row):
        row["command"] = cmd
        print(json.dumps(row), flush=True)

    def events(call, frames_per_call):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            call()
        b.record()
        torch.cuda.synchronize()
        return frames_per_call * steps / (a.elapsed_time(b) * 1e-3)

    def alternate(mixed, listed, frames_per_call):
        for _ in range(3):
            mixed()
            listed()
        m, l = [], []
        for _ in range(rounds):
            m.append(events(mixed, frames_per_call))
            l.append(events(listed, frames_per_call))
        return m, l

    def host_us(call, n=20):
        t = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        return round(float(np.median(t)), 1)

    for N, T in ((total, 1), (total // 4, 4)):
        Se, Sd = N // 10, N // 12  # streams per configuration
        enc_desc = [MIXED[q] for q in range(10) for _ in range(Se)]
        dec_desc = [MIXED[q] for q in range(12) for _ in range(Sd)]
        ne, nd = len(enc_desc), len(dec_desc)
        tile = lambda q, S: np.tile(base[q][:, :T], ((S + 63) // 64, 1, 1))[:S].reshape(-1)
        d_pcm = torch.from_numpy(np.concatenate([tile(q, Se) for q in range(10)])).cuda()
        # the decoder's input: its own mix encoded once (the 8 kHz streams with the spec flag that lets the encoder take them)
        src = pkg.Lc3Encoder.mixed(dec_desc, spec_flags=importlib.import_module("lc3-codec_amd.api").SPEC_8KHZ_ENCODE)
        d_in = torch.zeros(sum(T * d[2] for d in dec_desc), dtype=torch.uint8, device="cuda")
        src.encode_mixed(torch.from_numpy(np.concatenate([tile(q, Sd) for q in range(12)])).cuda(), d_in, T, stream=st)
        torch.cuda.synchronize()
        del src
        enc_m, enc_l = pkg.Lc3Encoder.mixed(enc_desc), pkg.Lc3Encoder.mixed(enc_desc)
        dec_m, dec_l = pkg.Lc3Decoder.mixed(dec_desc), pkg.Lc3Decoder.mixed(dec_desc)
        b_m, b_l = (torch.zeros(sum(T * d[2] for d in enc_desc), dtype=torch.uint8, device="cuda") for _ in range(2))
        p_m, p_l = (torch.zeros(sum(T * nf[q] * Sd for q in range(12)), dtype=torch.int16, device="cuda") for _ in range(2))
        che, chd = np.arange(ne, dtype=np.int32), np.arange(nd, dtype=np.int32)
        e_m = lambda: enc_m.encode_mixed(d_pcm, b_m, T, stream=st)
        e_l = lambda: enc_l.encode_mixed_list(che, d_pcm, b_l, T, stream=st)
        d_m = lambda: dec_m.decode_mixed(d_in, p_m, T, stream=st)
        d_l = lambda: dec_l.decode_mixed_list(chd, d_in, p_l, T, stream=st)
        e_m(), e_l(), d_m(), d_l()
        torch.cuda.synchronize()
        same = {"encode": bool(torch.equal(b_m, b_l)), "decode": bool(torch.equal(p_m, p_l))}
        for side, fm, fl, hm, hl, n in (("encode", e_m, e_l, enc_m, enc_l, ne), ("decode", d_m, d_l, dec_m, dec_l, nd)):
            m, l = alternate(fm, fl, n * T)
            mm, ml = float(np.mean(m)), float(np.mean(l))
            spread = (max(m) - min(m)) / mm
            row = {"figure": "parity", "side": side, "streams": n, "frames": T, "mixed_frames_per_s": round(mm), "mixed_list_frames_per_s": round(ml),
                   "list_over_mixed": round(ml / mm, 4), "mixed_spread": round(spread, 4), "mixed_rounds": [round(x) for x in m],
                   "list_rounds": [round(x) for x in l], "same_output": same[side], "allowance": ALLOWANCE,
                   "holds_allowance": bool(ml / mm >= ALLOWANCE - spread)}
            if not row["holds_allowance"]:  # which kernel lost it
                for name, h, f in (("mixed", hm, fm), ("mixed_list", hl, fl)):
                    h.timing(True)
                    for _ in range(10):
                        f()
                    row[name + "_kernel_ms_per_call"] = [round(x / 10, 4) for x in h.timing(False)[:-1]]
            emit(**row)
        if T == 1:
            emit(figure="host_us_per_call", n_list_encode=ne, n_list_decode=nd, encode_mixed=host_us(e_m), encode_mixed_list=host_us(e_l),
                 decode_mixed=host_us(d_m), decode_mixed_list=host_us(d_l))
            rng = np.random.default_rng(total)
            pcm_of = lambda c: base[c // Se][c % Se % 64, 0]  # encoder channel c: one frame
            boff = np.concatenate([[0], np.cumsum([d[2] for d in dec_desc])]).astype(np.int64)  # decoder channel c: its frame in d_in
            bytes_of = lambda l: d_in[torch.from_numpy(np.concatenate([np.arange(boff[c], boff[c + 1]) for c in l])).cuda()].contiguous()

            def subset_ticks(lists_e, lists_d, label, **extra):
                """every tick's buffers prepared once; the ticks take turns"""
                te = [(l, np.ascontiguousarray(l[: max(1, l.size // 100)]), torch.from_numpy(np.concatenate([pcm_of(int(c)) for c in l])).cuda(),
                       torch.zeros(int(sum(enc_desc[int(c)][2] for c in l)), dtype=torch.uint8, device="cuda")) for l in lists_e]
                td = [(l, np.ascontiguousarray(l[: max(1, l.size // 100)]), bytes_of(l),
                       torch.zeros(int(sum(nf[int(c) // Sd] for c in l)), dtype=torch.int16, device="cuda")) for l in lists_d]
                k = [0, 0]

                def tick_e():
                    l, fr, a, b = te[k[0] % len(te)]
                    k[0] += 1
                    enc_l.reset(fr)
                    enc_l.encode_mixed_list(l, a, b, 1, stream=st)

                def tick_d():
                    l, fr, a, b = td[k[1] % len(td)]
                    k[1] += 1
                    dec_l.reset(fr)
                    dec_l.decode_mixed_list(l, a, b, 1, stream=st)

                for f in (tick_e, tick_d):
                    for _ in range(3):
                        f()
                me, md = float(np.mean([l.size for l in lists_e])), float(np.mean([l.size for l in lists_d]))
                fe, fd = events(tick_e, me), events(tick_d, md)
                emit(figure=label, mean_n_list_encode=round(me), mean_n_list_decode=round(md), fresh_share=0.01, encode_frames_per_s=round(fe),
                     decode_frames_per_s=round(fd), encode_us_per_tick=round(me / fe * 1e6, 1), decode_us_per_tick=round(md / fd * 1e6, 1),
                     encode_host_us=host_us(tick_e), decode_host_us=host_us(tick_d), **extra)

            for part, div in (("subset_half", 2), ("subset_eighth", 8)):
                subset_ticks([rng.choice(ne, ne // div, replace=False).astype(np.int32) for _ in range(4)],
                             [rng.choice(nd, nd // div, replace=False).astype(np.int32) for _ in range(4)], part)
            due = lambda desc, i: np.array([c for c in range(len(desc)) if i % (3 if desc[c][1] == 7500 else 4) == 0], np.int32)
            keep = lambda a: rng.permutation(a[rng.random(a.size) >= 0.2]).astype(np.int32)
            le = [keep(due(enc_desc, i)) for i in range(12) if i % 3 == 0 or i % 4 == 0]
            ld = [keep(due(dec_desc, i)) for i in range(12) if i % 3 == 0 or i % 4 == 0]
            subset_ticks(le, ld, "clock_2_5_ms", ticks_per_period=len(le), n_list_encode=[int(l.size) for l in le])
        del enc_m, enc_l, dec_m, dec_l


if __name__ == "__main__":
    main()
