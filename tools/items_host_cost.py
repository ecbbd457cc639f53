#!/usr/bin/env python3
"""Host cost of the items, mc-items and views calls: wall time of one call that does not wait for the device (checks + plan + upload +
opt-ins + launches), the `host` figure of tools/items_batch.py for all six entry points.  The stream mix of tools/items_batch.py (equal
shares of the ten encodable configurations on the encoder, of all twelve on the decoder), one frame per item, mc items of one channel,
compact views; median of 20 calls after a warm-up call.  One JSON line, appended to `--out` (default profiles/items_host_refactor.jsonl) and
printed; LC3GPU_LIB names the library measured, so that two builds can be run alternately.
usage: python tools/items_host_cost.py [--items 65536] [--out FILE]"""
import importlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.items_batch import MIXED


def main():
    total = int(sys.argv[sys.argv.index("--items") + 1]) if "--items" in sys.argv else 65536
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "items_host_refactor.jsonl")
    import torch

    pkg = importlib.import_module("lc3-codec_amd")
    api = importlib.import_module("lc3-codec_amd.api")
    synth = importlib.import_module("lc3-codec_amd.synth")
    st = torch.cuda.current_stream().cuda_stream
    P = api._ptr
    L = pkg.load_library()
    nf = [pkg.Lc3Config(fs, us).nf for fs, us, _ in MIXED]
    base = [synth.make_pcm(64, 1, nf[k], MIXED[k][0], seed=51) for k in range(12)]
    row = {"figure": "host_us_per_call", "library": os.environ.get("LC3GPU_LIB") or "liblc3gpu.so",
           "command": "python tools/items_host_cost.py --items %d" % total}

    def host_us(call, n=20):
        call()
        t = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = call()
            t.append((time.perf_counter() - t0) * 1e6)
            assert rc == 0, rc
        torch.cuda.synchronize()
        return round(float(np.median(t)), 1)

    for side, n_cfg in (("encode", 10), ("decode", 12)):
        S = total // n_cfg
        desc = [MIXED[q] for q in range(n_cfg) for _ in range(S)]
        n = len(desc)
        d_pcm = torch.from_numpy(np.concatenate([np.tile(base[q], ((S + 63) // 64, 1, 1))[:S].reshape(-1) for q in range(n_cfg)])).cuda()
        d_bytes = torch.zeros(sum(d[2] for d in desc), dtype=torch.uint8, device="cuda")
        if side == "decode":
            src = pkg.Lc3Encoder.mixed(desc, spec_flags=api.SPEC_8KHZ_ENCODE)
            src.encode_mixed(d_pcm, d_bytes, 1, stream=st)
            torch.cuda.synchronize()
            del src
        po = np.concatenate([[0], np.cumsum([nf[MIXED.index(d)] for d in desc])])
        bo = np.concatenate([[0], np.cumsum([d[2] for d in desc])])
        items = api._item_list([(c, 1) for c in range(n)])
        mc = api._mc_item_list([(c, 1, 1) for c in range(n)])
        views = np.zeros(n, api.VIEW_DTYPE)
        views["channel"], views["n_frames"], views["pcm_stride"] = np.arange(n), 1, 1
        views["pcm_off"], views["byte_off"] = po[:-1], bo[:-1]
        row["n_items_" + side] = n
        for name, arr in (("items", items), ("mc_items", mc), ("views", views)):
            if side == "encode":
                h = pkg.Lc3Encoder.mixed(desc)
                if name == "views":
                    call = lambda: L.lc3gpu_encode_mixed_views(h._h, P(arr), n, P(d_pcm), d_pcm.numel(), P(d_bytes), d_bytes.numel(), P(st))
                else:
                    call = lambda: getattr(L, "lc3gpu_encode_mixed_" + name)(h._h, P(arr), n, P(d_pcm), P(d_bytes), P(st))
            else:
                h = pkg.Lc3Decoder.mixed(desc)
                if name == "views":
                    call = lambda: L.lc3gpu_decode_mixed_views(h._h, P(arr), n, P(d_bytes), d_bytes.numel(), None, 0, P(d_pcm), d_pcm.numel(), P(st))
                else:
                    call = lambda: getattr(L, "lc3gpu_decode_mixed_" + name)(h._h, P(arr), n, P(d_bytes), None, P(d_pcm), P(st))
            row["%s_mixed_%s" % (side, name)] = host_us(call)
            assert h.pair_timeouts() == 0
            del h
    line = json.dumps(row)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
