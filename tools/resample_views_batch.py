#!/usr/bin/env python3
"""lc3gpu_resample_mixed_views at a mixing server's tick size: half the streams 16 -> 48 kHz (a headset into a 48 kHz room), half 48 -> 16 kHz
(the room's mix back to it), all 10 ms, `--frames` frames per tick in two shapes -- streams x 1 frame and a quarter of the streams x 4 frames
--, PCM rings of 8 slots of 480 samples per stream on both sides (tools/views_batch.py), one process, one caller stream.  Before anything is
timed the first call's ring is compared with the numpy model (tests/resample_lib.py) on a sample of the streams.  One JSON line per figure,
written to `--out` (default profiles/resample_views_measurements.jsonl) and printed:
  resample_call   ms per call by GPU events over `--steps` calls queued back to back (what a tick pays), the host's share -- the wall time the
                  same calls take to RETURN: check, plan, upload and launch being queued --, the check and plan alone (the calls refused at
                  their last view, so that nothing is queued), the bytes a call must move at the least -- every input sample read once and
                  every output sample written once -- and that figure over the call time against the copy figure of
                  profiles/r04_valu_ceiling.json (bench.py's measured_copy_GBs: bytes read plus bytes written).
The kernel's time alone is no figure of this tool: it is read from a kernel trace of a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/resample_views_batch.py --steps 5 --rounds 1 --out /dev/null); the committed record
holds those lines (figure "kernel_trace") behind the tool's own, appended by hand.
usage: python tools/resample_views_batch.py [--frames 65536] [--steps 50] [--rounds 3] [--out FILE]"""
import importlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLOTS, SLOT_PCM = 8, 480
KINDS = [(16000, 48000, 10000), (48000, 16000, 10000)]


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    total, steps, rounds = arg("--frames", 65536), arg("--steps", 50), arg("--rounds", 3)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "resample_views_measurements.jsonl")
    cmd = "python tools/resample_views_batch.py --frames %d --steps %d --rounds %d" % (total, steps, rounds)
    open(out_path, "w").close()  # a run replaces the file
    import torch

    pkg = importlib.import_module("lc3-codec_amd")
    api = importlib.import_module("lc3-codec_amd.api")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resample_lib as R

    st = torch.cuda.current_stream().cuda_stream
    P = api._ptr
    L = pkg.load_library()
    with open(os.path.join(ROOT, "profiles", "r04_valu_ceiling.json")) as f:
        copy_gbs = float(json.load(f)["copy"]["GBs_read_plus_write"])
    spw = api.resampler_plan_info()[0]

    def emit(**row):
        row["command"] = cmd
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")

    for streams_total, T in ((total, 1), (total // 4, 4)):
        n_ch = streams_total // 16 * 16  # (the mixer record's streams: whole rooms of 8 of either kind)
        n_ch = min(n_ch, 65520 if T == 1 else 16320)
        desc = [KINDS[c & 1] for c in range(n_ch)]
        nf_in = np.array([d[0] // 100 for d in desc])
        nf_out = np.array([d[1] // 100 for d in desc])
        rng = np.random.default_rng(5)
        slot0 = rng.integers(0, SLOTS - T + 1, n_ch)
        first = np.arange(n_ch) * SLOTS + slot0
        ring = n_ch * SLOTS * SLOT_PCM
        vin = api._view_list([dict(channel=c, n_frames=T, pcm_off=int(first[c] * SLOT_PCM), pcm_pitch=SLOT_PCM, byte_off=0) for c in range(n_ch)])
        vout = vin.copy()
        pcm_in = rng.integers(-32768, 32768, ring).astype(np.int16)
        d_in = torch.from_numpy(pcm_in).cuda()
        d_out = torch.full((ring,), 77, dtype=torch.int16, device="cuda")
        rs = pkg.Lc3Resampler(desc, n_ch)

        def call():
            return L.lc3gpu_resample_mixed_views(rs._h, P(vin), P(d_in), ring, P(vout), P(d_out), ring, n_ch, P(st))

        # the same lists, refused at the last view (its output begins two samples before the ring ends): the host's check of every view,
        # nothing queued
        vbad = vout.copy()
        vbad["pcm_off"][-1] = ring - 2
        refused = lambda: L.lc3gpu_resample_mixed_views(rs._h, P(vin), P(d_in), ring, P(vbad), P(d_out), ring, n_ch, P(st))
        assert call() == 0 and refused() == -3
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        mod = R.Model(desc)
        some = rng.choice(n_ch, 64, replace=False)
        want = mod.call(vin[some], pcm_in, vout[some], np.full(ring, 77, np.int16))
        for c in some:
            lo, hi = int(first[c]) * SLOT_PCM, (int(first[c]) + T) * SLOT_PCM
            assert np.array_equal(got[lo:hi], want[lo:hi]), "stream %d differs from the model" % c
        moved = int(((nf_in + nf_out) * T * 2).sum())
        wgs = int((-(-(nf_out * T) // spw)).sum())
        for _ in range(3):
            call()
        ev, host, plan = [], [], []
        for _ in range(rounds):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            for _ in range(steps):
                call()
            t1 = time.perf_counter()
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b) / steps)
            host.append((t1 - t0) * 1e3 / steps)
            t0 = time.perf_counter()
            for _ in range(steps):
                refused()
            plan.append((time.perf_counter() - t0) * 1e3 / steps)
        m_ev, m_host, m_plan = float(np.mean(ev)), float(np.mean(host)), float(np.mean(plan))
        emit(figure="resample_call", streams=n_ch, frames=T, frames_per_call=n_ch * T, mix="half 16->48 kHz, half 48->16 kHz, 10 ms", workgroups=wgs,
             call_ms=round(m_ev, 4), call_rounds_ms=[round(v, 4) for v in ev], call_spread=round((max(ev) - min(ev)) / m_ev, 4),
             host_ms_until_the_calls_return=round(m_host, 4), host_check_ms=round(m_plan, 4), host_share_of_call=round(m_host / m_ev, 3),
             bytes_moved_per_call_at_least=moved, call_GBs=round(moved / (m_ev * 1e-3) / 1e9, 1), measured_copy_GBs=copy_gbs,
             call_share_of_copy=round(moved / (m_ev * 1e-3) / 1e9 / copy_gbs, 3))
        rs.close()


if __name__ == "__main__":
    main()
