#!/usr/bin/env python3
"""The list calls (lc3gpu_encode_list / lc3gpu_decode_list) against the uniform ones at 48 kHz / 10 ms / 150 bytes, state carried, one
process, one caller stream, GPU events over `--steps` calls per measurement, the two sides of every comparison alternating.  One JSON line:
  parity     list = 0 .. n-1 against lc3gpu_encode and lc3gpu_decode at 65 536 x 1 and 16 384 x 4: frames/s of both sides (mean of
             `--rounds` alternating measurements), their ratio, the spread between the repeated uniform measurements, and whether the ratio
             holds 0.952 (what the sized call was accepted with) less that spread; the per-kernel times of both sides when it does not;
  host       wall time of one call that does not wait for the device (check + list upload + launches) at n_list = 65 536, beside the
             same for lc3gpu_encode / lc3gpu_decode (median over calls with an idle device);
  subset     a random half and a random eighth of 65 536 channels per tick, one frame, 1 % of the listed channels reset before the tick:
             frames/s.
usage: python tools/list_batch.py [--steps 50] [--rounds 3]"""
import importlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ALLOWANCE = 0.952  # profiles/vbr_measurements.jsonl: the sized call over the uniform call, as accepted


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    steps, rounds = arg("--steps", 50), arg("--rounds", 3)
    import torch

    pkg = importlib.import_module("lc3-codec_amd")
    synth = importlib.import_module("lc3-codec_amd.synth")
    FS, US, nf, nbytes, N = pkg.SamplingFrequency.Hz48000, pkg.FrameDuration.TenMs, 480, 150, 65536
    base = synth.make_pcm(2048, 4, nf, 48000)
    st = torch.cuda.current_stream().cuda_stream

    def events(call, frames_per_call):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            call()
        b.record()
        torch.cuda.synchronize()
        return frames_per_call * steps / (a.elapsed_time(b) * 1e-3)

    def alternate(uniform, listed, frames_per_call):
        for _ in range(3):
            uniform()
            listed()
        u, l = [], []
        for _ in range(rounds):
            u.append(events(uniform, frames_per_call))
            l.append(events(listed, frames_per_call))
        return u, l

    def host_us(call, n=20):
        t = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        return round(float(np.median(t)), 1)

    out = {"config": "48000 Hz / 10000 us / %d bytes, one caller stream, %d timed calls x %d alternating rounds" % (nbytes, steps, rounds),
           "allowance": ALLOWANCE, "parity": [], "host_us_per_call": {}, "subset": []}
    for S, T in ((N, 1), (16384, 4)):
        pcm = np.ascontiguousarray(np.tile(base[:, :T], (S // 2048, 1, 1)))
        d_pcm = torch.from_numpy(pcm).cuda()
        ch = np.arange(S, dtype=np.int32)
        enc_u, enc_l = pkg.Lc3Encoder(S, US, FS), pkg.Lc3Encoder(S, US, FS)
        dec_u, dec_l = pkg.Lc3Decoder(S, US, FS), pkg.Lc3Decoder(S, US, FS)
        b_u, b_l = (torch.zeros((S, T, nbytes), dtype=torch.uint8, device="cuda") for _ in range(2))
        p_u, p_l = (torch.zeros((S, T, nf), dtype=torch.int16, device="cuda") for _ in range(2))
        e_u = lambda: enc_u.encode(d_pcm, b_u, nbytes, T, stream=st)
        e_l = lambda: enc_l.encode_list(ch, d_pcm, b_l, nbytes, T, stream=st)
        e_u(), e_l()
        torch.cuda.synchronize()
        same_e = bool(torch.equal(b_u, b_l))
        d_u = lambda: dec_u.decode(b_u, p_u, nbytes, T, stream=st)
        d_l = lambda: dec_l.decode_list(ch, b_u, p_l, nbytes, T, stream=st)
        d_u(), d_l()
        torch.cuda.synchronize()
        same_d = bool(torch.equal(p_u, p_l))
        for side, fu, fl, same, hu, hl in (("encode", e_u, e_l, same_e, enc_u, enc_l), ("decode", d_u, d_l, same_d, dec_u, dec_l)):
            u, l = alternate(fu, fl, S * T)
            mu, ml = float(np.mean(u)), float(np.mean(l))
            spread = (max(u) - min(u)) / mu
            row = {"side": side, "streams": S, "frames": T, "uniform_frames_per_s": round(mu), "list_frames_per_s": round(ml),
                   "list_over_uniform": round(ml / mu, 4), "uniform_spread": round(spread, 4), "uniform_rounds": [round(x) for x in u],
                   "list_rounds": [round(x) for x in l], "same_output": same, "holds_allowance": bool(ml / mu >= ALLOWANCE - spread)}
            if not row["holds_allowance"]:  # which kernel lost it
                for name, h, f in (("uniform", hu, fu), ("list", hl, fl)):
                    h.timing(True)
                    for _ in range(10):
                        f()
                    row[name + "_kernel_ms_per_call"] = [round(x / 10, 4) for x in h.timing(False)[:-1]]
            out["parity"].append(row)
        if S == N:
            out["host_us_per_call"] = {"n_list": S, "encode": host_us(e_u), "encode_list": host_us(e_l), "decode": host_us(d_u),
                                       "decode_list": host_us(d_l)}
            # the case without a counterpart: a random subset per tick, 1 % of it reset before the tick (eight lists taking turns)
            rng = np.random.default_rng(65536)
            for part, n in (("half", S // 2), ("eighth", S // 8)):
                lists = [rng.choice(S, n, replace=False).astype(np.int32) for _ in range(8)]
                fresh = [np.ascontiguousarray(x[: max(1, n // 100)]) for x in lists]
                d_p, d_b, d_o = d_pcm[:n], b_u[:n], p_l[:n]
                k = [0, 0]

                def tick_e():
                    i = k[0] % 8
                    k[0] += 1
                    enc_l.reset(fresh[i])
                    enc_l.encode_list(lists[i], d_p, b_l[:n], nbytes, 1, stream=st)

                def tick_d():
                    i = k[1] % 8
                    k[1] += 1
                    dec_l.reset(fresh[i])
                    dec_l.decode_list(lists[i], d_b, d_o, nbytes, 1, stream=st)

                for f in (tick_e, tick_d):
                    for _ in range(3):
                        f()
                out["subset"].append({"part": part, "n_list": n, "fresh_per_tick": int(fresh[0].size),
                                      "encode_list_frames_per_s": round(events(tick_e, n)), "decode_list_frames_per_s": round(events(tick_d, n)),
                                      "encode_list_host_us": host_us(tick_e), "decode_list_host_us": host_us(tick_d)})
        del enc_u, enc_l, dec_u, dec_l
    print(json.dumps(out))


if __name__ == "__main__":
    main()
