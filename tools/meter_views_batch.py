#!/usr/bin/env python3
"""lc3gpu_measure_mixed_views at a mixing server's tick size: 48 kHz / 10 ms streams, `--frames` frames per tick in the two shapes the
resampler was timed at -- streams x 1 frame and a quarter of the streams x 4 frames --, a PCM ring of 8 slots of 480 samples per stream
(tools/views_batch.py), activity bytes and records on, one process, one caller stream.  Before anything is timed the first call's records
are compared with the model (tests/meter_lib.py) on a sample of the streams.  One JSON line per figure, written to `--out` (default
profiles/meter_views_measurements.jsonl) and printed:
  meter_call   ms per call by GPU events over `--steps` calls queued back to back (what a tick pays); the host's share -- the wall time the
               same calls take to RETURN: check, rows, upload and launch being queued --; the check alone (the calls refused at their last
               view, so that nothing is queued); the DEVICE's share -- upload and kernel of as many calls as the ring has slots, queued
               behind a kernel that keeps the stream busy until all of them are queued, so that the host bounds nothing --; the bytes a call
               must move at the least -- every sample read once, 32 + 1 bytes written per frame -- and that figure over the device time
               against the copy figure of profiles/r04_valu_ceiling.json (bench.py's measured_copy_GBs: bytes read plus bytes written).
usage: python tools/meter_views_batch.py [--frames 65536] [--steps 50] [--rounds 3] [--out FILE]"""
import importlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLOTS, SLOT_PCM, NF = 8, 480, 480


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d
    total, steps, rounds = arg("--frames", 65536), arg("--steps", 50), arg("--rounds", 3)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "meter_views_measurements.jsonl")
    cmd = "python tools/meter_views_batch.py --frames %d --steps %d --rounds %d" % (total, steps, rounds)
    open(out_path, "w").close()  # a run replaces the file
    import torch

    pkg = importlib.import_module("lc3-codec_amd")
    api = importlib.import_module("lc3-codec_amd.api")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import meter_lib as ML

    st = torch.cuda.current_stream().cuda_stream
    P = api._ptr
    L = pkg.load_library()
    with open(os.path.join(ROOT, "profiles", "r04_valu_ceiling.json")) as f:
        copy_gbs = float(json.load(f)["copy"]["GBs_read_plus_write"])
    wpw, lanes, ring_slots, _ = api.meter_plan_info()

    def emit(**row):
        row["command"] = cmd
        line = json.dumps(row)
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")

    for streams_total, T in ((total, 1), (total // 4, 4)):
        n_ch = min(streams_total // 16 * 16, 65520 if T == 1 else 16320)  # (the resampler record's streams)
        desc = [ML.desc(48000, 10000, attack=16384, release=1024, threshold=1 << 18, hang=20) for _ in range(n_ch)]
        rng = np.random.default_rng(5)
        slot0 = rng.integers(0, SLOTS - T + 1, n_ch)
        first = np.arange(n_ch) * SLOTS + slot0
        ring = n_ch * SLOTS * SLOT_PCM
        views = api._view_list([dict(channel=c, n_frames=T, pcm_off=int(first[c] * SLOT_PCM), pcm_pitch=SLOT_PCM, byte_off=0, flag_off=c * T)
                                for c in range(n_ch)])
        pcm = (rng.integers(-32768, 32768, ring) >> rng.integers(0, 12, ring // SLOT_PCM).repeat(SLOT_PCM)).astype(np.int16)  # (loud and quiet slots)
        d_pcm = torch.from_numpy(pcm).cuda()
        n_out = n_ch * T
        d_active = torch.full((n_out,), 0xA5, dtype=torch.uint8, device="cuda")
        d_levels = torch.full((n_out * 32,), 0x5C, dtype=torch.uint8, device="cuda")
        mt = pkg.Lc3Meter(desc, n_ch)

        def call():
            return L.lc3gpu_measure_mixed_views(mt._h, P(views), n_ch, P(d_pcm), ring, P(d_active), n_out, P(d_levels), n_out, P(st))

        # the same list, refused at the last view (it begins two samples before the ring ends): the host's check of every view, nothing queued
        vbad = views.copy()
        vbad["pcm_off"][-1] = ring - 2
        refused = lambda: L.lc3gpu_measure_mixed_views(mt._h, P(vbad), n_ch, P(d_pcm), ring, P(d_active), n_out, P(d_levels), n_out, P(st))
        assert call() == 0 and refused() == -3
        torch.cuda.synchronize()
        got_a, got_lv = d_active.cpu().numpy(), d_levels.cpu().numpy().view(api.LEVEL_DTYPE)
        some = np.sort(rng.choice(n_ch, 64, replace=False))
        want_a, want_lv = ML.Model(desc).call(views[some], pcm, np.full(n_out, 0xA5, np.uint8), np.zeros(n_out, api.LEVEL_DTYPE))
        for c in some:
            lo, hi = int(c) * T, int(c) * T + T
            assert np.array_equal(got_lv[lo:hi], want_lv[lo:hi]) and np.array_equal(got_a[lo:hi], want_a[lo:hi]), "stream %d differs from the model" % c
        moved = n_out * (NF * 2 + 32 + 1)
        for _ in range(3):
            call()
        ev, host, plan, devt = [], [], [], []
        blocker = torch.randn(4096, 4096, device="cuda")
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
            # the device's share: as many calls as the ring has slots, all queued while the stream is still busy with the blocker
            torch.cuda.synchronize()
            x = blocker
            for _ in range(12):
                x = x @ blocker / 64.0
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ring_slots):
                call()
            b.record()
            still_busy = not a.query()  # (the blocker had not finished when the last call was queued: the host bounded nothing)
            torch.cuda.synchronize()
            if still_busy:
                devt.append(a.elapsed_time(b) / ring_slots)
        m_ev, m_host, m_plan = float(np.mean(ev)), float(np.mean(host)), float(np.mean(plan))
        m_dev = float(np.mean(devt)) if devt else None
        emit(figure="meter_call", streams=n_ch, frames=T, frames_per_call=n_out, mix="48 kHz, 10 ms, activity bytes and records", workgroups=-(-n_ch // wpw),
             call_ms=round(m_ev, 4), call_rounds_ms=[round(v, 4) for v in ev], call_spread=round((max(ev) - min(ev)) / m_ev, 4),
             host_ms_until_the_calls_return=round(m_host, 4), host_check_ms=round(m_plan, 4), host_share_of_call=round(m_host / m_ev, 3),
             device_ms_upload_and_kernel=None if m_dev is None else round(m_dev, 4), device_rounds_ms=[round(v, 4) for v in devt],
             bytes_moved_per_call_at_least=moved, measured_copy_GBs=copy_gbs,
             device_GBs=None if m_dev is None else round(moved / (m_dev * 1e-3) / 1e9, 1),
             device_share_of_copy=None if m_dev is None else round(moved / (m_dev * 1e-3) / 1e9 / copy_gbs, 3))
        mt.close()


if __name__ == "__main__":
    main()
