#!/usr/bin/env python3
"""Frame inspection (lc3gpu_inspect) on 65 536 frames of 48 kHz / 10 ms / 150 bytes, timed with GPU events on one caller stream, beside the
decoder's parse stage on the same frames in the same process.  Appends one JSON line to profiles/inspect_measurements.jsonl:
  (a) clean frames (from the oracle encoder) and (b) the same with 10 % of them damaged (flipped bits, random tails; ~5 % of all frames
      then fail): inspection frames/s and ms per call, records of a sample checked against the oracle;
  (c) the decoder's parse-stage kernel time per 65 536 frames (lc3gpu_decoder_timing_kernels: 16 384 streams x 4 frames, (a)'s bytes);
  (d) with --rocprof: lc3_inspect_kernel's mean duration on (a) from a separate `rocprofv3 --kernel-trace --stats` run of this script
      (--child: the clean calls only, nothing written).
usage: python tools/inspect_batch.py [--steps 50] [--rocprof] [--out FILE]"""
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
S, T, NB = 16384, 4, 150


def frames():
    import inspect_lib as I
    import oracle_lib as O

    synth = importlib.import_module("lc3-codec_amd.synth")
    base = O.encode_batch(synth.make_pcm(2048, T, 480, 48000), NB, threads=16)
    clean = np.ascontiguousarray(np.tile(base, (S // 2048, 1, 1))).reshape(S * T, NB)
    damaged, _ = I.damage(clean, np.random.default_rng(10), frac=0.10)
    return clean, damaged


def rocprof_kernel_ms(steps):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "trace", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--steps", str(steps)]
        subprocess.run(cmd, check=True, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                if "lc3_inspect_kernel" in row["Name"]:
                    return {"calls": int(row["Calls"]), "mean_ms": round(float(row["AverageNs"]) * 1e-6, 4),
                            "min_ms": round(float(row["MinNs"]) * 1e-6, 4), "max_ms": round(float(row["MaxNs"]) * 1e-6, 4)}
    return None


def main():
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 50
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "inspect_measurements.jsonl")
    child = "--child" in sys.argv
    import torch
    import inspect_lib as I

    pkg = importlib.import_module("lc3-codec_amd")
    clean, damaged = frames()
    st = torch.cuda.current_stream().cuda_stream
    n = S * T
    d_info = torch.zeros((n, 32), dtype=torch.int32, device="cuda")

    def timed(call, k):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    res = {"config": "48000 Hz / 10000 us, %d frames x %d bytes, one caller stream, %d timed calls" % (n, NB, steps)}
    for tag, data in (("clean", clean),) if child else (("clean", clean), ("damaged_10pct", damaged)):
        d_in = torch.from_numpy(data).cuda()
        call = lambda: pkg.inspect(10000, 48000, d_in, d_info, NB, n, stream=st)
        ms = timed(call, steps)
        if child:
            continue
        got = d_info.cpu().numpy()
        sample = np.random.default_rng(1).choice(n, 4096, replace=False)
        ref = I.oracle_records(48000, 10000, data[sample])
        res[tag] = {"ms_per_call": round(ms, 4), "frames_per_s": round(n / (ms * 1e-3)), "status_nonzero": int((got[:, 0] != 0).sum()),
                    "sample_checked": len(sample), "sample_differing": int((got[sample] != ref).any(1).sum())}
    if child:
        return
    # the decoder's parse stage on (a)'s bytes, same process
    dec = pkg.Lc3Decoder(S, 10000, 48000)
    d_in = torch.from_numpy(clean.reshape(S, T, NB)).cuda()
    d_pcm = torch.zeros((S, T, 480), dtype=torch.int16, device="cuda")
    for _ in range(3):
        dec.decode(d_in, d_pcm, NB, T, stream=st)
    torch.cuda.synchronize()
    dec.timing_kernels(True)
    for _ in range(steps):
        dec.decode(d_in, d_pcm, NB, T, stream=st)
    parse, recon, tns, synth_ms, calls = dec.timing_kernels(False)
    res["decoder_parse_stage"] = {"parse_ms_per_call": round(parse / calls, 4), "recon_ms_per_call": round(recon / calls, 4),
                                  "tns_ms_per_call": round(tns / calls, 4), "synthesis_ms_per_call": round(synth_ms / calls, 4),
                                  "calls": calls}
    res["inspect_over_parse_time"] = round(res["clean"]["ms_per_call"] / res["decoder_parse_stage"]["parse_ms_per_call"], 3)
    dec.close()
    if "--rocprof" in sys.argv:
        res["rocprof_lc3_inspect_kernel"] = rocprof_kernel_ms(steps)
    line = json.dumps(res)
    print(line)
    with open(out_path, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
