"""The stream ordering of lc3gpu_pipeline against a happens-before model (tests/hb/lc3_pipeline_hb_main.cpp), on the CPU.

The pipeline object (lc3-codec_amd/csrc/lc3gpu_pipeline.cpp) is ordering and nothing else, and a GPU test that compares results after a
wait passes with a wait missing almost every time.  Here the pipeline's own source is compiled with g++ and linked with a fake HIP runtime
and fake codec handles that execute nothing and log everything; scripted and seeded random caller programs, all legal under the contract
of include/lc3gpu.h, run under three device-progress policies, and a checker asserts over the trace that conflicting accesses are ordered
and that wait / join / mark mean what the header says.  The program has its own main, is built with -fsanitize=address,undefined (runtimes
linked statically) and runs as a child process; nothing of it is loaded into Python and no process of it opens a GPU.

A green model proves nothing by itself: the same program is also built from MUTANTS of the pipeline source -- one textual replacement
each, applied to a temporary copy, the replaced text asserted to occur exactly once -- and every mutant must be rejected."""
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPELINE_SRC = os.path.join(ROOT, "lc3-codec_amd", "csrc", "lc3gpu_pipeline.cpp")
MAIN_SRC = os.path.join(ROOT, "tests", "hb", "lc3_pipeline_hb_main.cpp")
N_RANDOM = 300  # seeded random caller programs, each under the three policies

# what the pipeline's object file leaves undefined, and the fakes therefore define: exactly these
HIP_CALLS = {"hipDeviceGetStreamPriorityRange", "hipEventCreateWithFlags", "hipEventDestroy", "hipEventQuery", "hipEventRecord",
             "hipEventSynchronize", "hipGetDevice", "hipGetLastError", "hipSetDevice", "hipStreamCreateWithPriority", "hipStreamDestroy",
             "hipStreamSynchronize", "hipStreamWaitEvent"}
LC3GPU_CALLS = {"lc3gpu_config", "lc3gpu_device_count", "lc3gpu_encoder_create", "lc3gpu_decoder_create", "lc3gpu_encoder_create_mixed",
                "lc3gpu_decoder_create_mixed", "lc3gpu_encoder_destroy", "lc3gpu_decoder_destroy", "lc3gpu_encoder_bind_stream",
                "lc3gpu_decoder_bind_stream", "lc3gpu_encode", "lc3gpu_decode", "lc3gpu_encode_mixed", "lc3gpu_decode_mixed",
                "lc3gpu_encoder_reset", "lc3gpu_decoder_reset", "lc3gpu_encoder_pair_pending", "lc3gpu_decoder_pair_pending"}

ENC_LAUNCH = ("            rc = p->mixed ? lc3gpu_encode_mixed(q.enc, d_pcm + pcm_off, bytes, n_frames, q.s_enc)\n"
              "                          : lc3gpu_encode(q.enc, d_pcm + pcm_off, bytes, nbytes, n_frames, q.s_enc);\n"
              "            if (rc) return rc;\n")
ENC_SLOT = "            const int b = (int)(q.n_enc & 1ull);\n"
ENC_RECORD = "            PL_HIP(p, hipEventRecord(q.enc_done[b], q.s_enc));\n"

# name -> (the text replaced, which occurs exactly once; its replacement)
MUTANTS = {
    "no wait for the decoders before the encode": (
        "if ((rc = wait_for_other_role(p, q.s_enc, bytes, bytes_end, q.dec_done, q.dec_rec, q.bytes_lo, q.bytes_hi, q.n_dec, &behind_newest)) != 0) return rc;", ""),
    "no wait for the encoders before the decode": (
        "if ((rc = wait_for_other_role(p, q.s_dec, bytes, bytes_end, q.enc_done, q.enc_rec, q.ebytes_lo, q.ebytes_hi, q.n_enc, &behind_newest)) != 0) return rc;", ""),
    "no fallback for dropped records": ("if (!any && count > 2 && rec[older]) return wait_unless_done(p, s, ev[older]);", ""),
    "newer and older slots swapped": ("const int newer = (int)((count - 1) & 1ull), older = newer ^ 1;",
                                      "const int older = (int)((count - 1) & 1ull), newer = older ^ 1;"),
    "overlaps means equal start pointers": ("{ return a_lo < b_hi && b_lo < a_hi; }", "{ return a_lo == b_lo && a_hi && b_hi; }"),
    "no follow_wait on the decoder side": ("if ((rc = follow_wait(p, q.s_dec)) != 0) return rc;", ""),
    "hipEventQuery shortcut inverted": ("if (hipEventQuery(ev) == hipSuccess) return LC3GPU_OK;", "if (hipEventQuery(ev) != hipSuccess) return LC3GPU_OK;"),
    "enc_done recorded before the launch": (ENC_LAUNCH + ENC_SLOT + ENC_RECORD, ENC_SLOT + ENC_RECORD + ENC_LAUNCH),
    "wait synchronises the decoders only": ("if (q.last_enc >= 0) PL_HIP(p, hipEventSynchronize(q.enc_done[q.last_enc]));", ""),
    "join omits the encoder events": ("if (q.last_enc >= 0) PL_HIP(p, hipStreamWaitEvent((hipStream_t)hip_stream, q.enc_done[q.last_enc], 0));", ""),
    "mark on s_dec whenever the group has ever decoded": ("if (q.last_enc >= 0 && q.last_dec >= 0 && !q.dec_covers_enc) {", "if (false) {"),
    "encoders ignore the other groups after a change of geometry": ("if (q.enc_epoch != p->epoch) {", "if (false) {"),
    "decoders ignore the other groups after a change of geometry": ("if (q.dec_epoch != p->epoch) {", "if (false) {"),
    "a fifth byte buffer pushes one out of the list": ("if (fits && !known && p->geo_n == 4) fits = false;", "if (fits && !known && p->geo_n == 4) p->geo_n = 3;"),
    "n_frames and nbytes no part of the geometry": ("bool fits = p->geo_n == 0 || (n_frames == p->geo_n_frames && nbytes == p->geo_nbytes);", "bool fits = true;"),
    "encoder pair flags not looked at first": ("if ((what & 1) && lc3gpu_encoder_pair_pending(q.enc) > 0) {", "if (false) {"),
    "decoder pair flags not looked at first": ("if ((what & 2) && lc3gpu_decoder_pair_pending(q.dec) > 0) {", "if (false) {"),
    "PCM alignment left to the handles": (
        "if (((what & 1) && ((uintptr_t)d_pcm & 3u) != 0) || ((what & 2) && ((uintptr_t)d_pcm_out & 3u) != 0)) return LC3GPU_EINVAL;", ""),
    "nbytes left to the handles": ("if (!p->mixed && (nbytes < ((what & 1) ? 20 : 1) || nbytes > 400)) return LC3GPU_ELENGTH;", ""),
    "a decode alone held to the encoder's nbytes": ("(nbytes < ((what & 1) ? 20 : 1) || nbytes > 400)", "(nbytes < 20 || nbytes > 400)"),
    "given boundaries with a defaulted or clamped group count": ("if (group_first && (n_groups == 0 || n_groups > n_streams)) return LC3GPU_EINVAL;", ""),
}


def _rocm_include():
    hipcc = shutil.which("hipcc")
    roots = [os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), os.path.dirname(os.path.dirname(os.path.realpath(hipcc))) if hipcc else None,
             "/opt/rocm"]
    for r in roots:
        if r and os.path.exists(os.path.join(r, "include", "hip", "hip_runtime.h")):
            return os.path.join(r, "include")
    pytest.fail("no ROCm headers found (ROCM_PATH, beside hipcc, /opt/rocm)")


def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)


@pytest.fixture(scope="module")
def model():
    """{variant: (exit status, output)} for the source as it is (variant None) and for every mutant, and the undefined symbols of the
    pipeline's object file"""
    with open(PIPELINE_SRC) as f:
        text = f.read()
    sources = {None: text}
    for name, (old, new) in MUTANTS.items():
        assert text.count(old) == 1, "mutant %r: its text occurs %d times in lc3gpu_pipeline.cpp" % (name, text.count(old))
        sources[name] = text.replace(old, new)
    inc = _rocm_include()
    base = ["g++", "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-Wno-unknown-pragmas", "-Wno-unused-result"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    san_link = san + ["-static-libasan", "-static-libubsan"]  # (the program is whole, whatever else a machine loads into every process)
    jobs = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    with tempfile.TemporaryDirectory() as tmp:
        # the mutants are copies under the same relative path, so that their #include "../../include/lc3gpu.h" finds this tree's header
        os.makedirs(os.path.join(tmp, "include"))
        shutil.copy(os.path.join(ROOT, "include", "lc3gpu.h"), os.path.join(tmp, "include", "lc3gpu.h"))
        names = list(sources)
        dirs = {}
        for i, name in enumerate(names):
            d = os.path.join(tmp, "v%02d" % i, "csrc")
            os.makedirs(d)
            with open(os.path.join(d, "lc3gpu_pipeline.cpp"), "w") as f:
                f.write(sources[name])
            dirs[name] = d
        # one probe decides whether this compiler can link the sanitizer runtimes; without them the model still runs, unsanitized
        probe = os.path.join(tmp, "probe.cpp")
        with open(probe, "w") as f:
            f.write("int main() { return 0; }\n")
        probe_run = _run(["g++"] + san_link + ["-o", os.path.join(tmp, "probe"), probe])
        sanitized = probe_run.returncode == 0
        cflags, lflags = base + (san if sanitized else []), (san_link if sanitized else [])
        main_obj = os.path.join(tmp, "main.o")

        def compile_main():
            return _run(cflags + ["-c", "-o", main_obj, MAIN_SRC])

        def compile_variant(name):
            d = dirs[name]
            return _run(cflags + ["-c", "-o", os.path.join(d, "pipeline.o"), os.path.join(d, "lc3gpu_pipeline.cpp")])

        def link_and_run(name):
            d = dirs[name]
            r = _run(["g++"] + lflags + ["-o", os.path.join(d, "hb"), main_obj, os.path.join(d, "pipeline.o")])
            if r.returncode != 0:
                return None, r.stdout
            r = _run([os.path.join(d, "hb"), str(N_RANDOM)])
            return r.returncode, r.stdout

        with ThreadPoolExecutor(max_workers=jobs) as pool:
            fm = pool.submit(compile_main)
            compiled = dict(zip(names, pool.map(compile_variant, names)))
            r = fm.result()
            assert r.returncode == 0, r.stdout[-3000:]
            for name in names:
                assert compiled[name].returncode == 0, "%r does not compile:\n%s" % (name, compiled[name].stdout[-3000:])
            results = dict(zip(names, pool.map(link_and_run, names)))
        undefined = set(_run(["nm", "-u", os.path.join(dirs[None], "pipeline.o")]).stdout.split())
    return {"results": results, "undefined": undefined, "sanitized": sanitized, "probe": probe_run.stdout}


def test_the_program_ran_under_address_and_undefined_behaviour_sanitizers(model):
    """where the compiler cannot link the sanitizer runtimes the model above still runs, unsanitized, and this test says so in the report"""
    if not model["sanitized"]:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + (model["probe"].strip().splitlines() or ["?"])[-1])
    assert model["results"][None][0] == 0


def _failed_scenarios(output):
    """{scenario: [(policy, first violation)]} of one run's output"""
    out = {}
    for m in re.finditer(r"^FAIL (\S+) policy=(\S+): (.*)$", output, re.M):
        out.setdefault(m.group(1), []).append((m.group(2), m.group(3)))
    return out


def test_the_fakes_define_exactly_what_the_pipeline_object_leaves_undefined(model):
    names = {s for s in model["undefined"] if s.startswith(("hip", "lc3gpu_"))}
    assert names == HIP_CALLS | LC3GPU_CALLS, sorted(names ^ (HIP_CALLS | LC3GPU_CALLS))


def test_the_source_as_it_is_passes_every_scenario_under_all_three_policies(model):
    rc, out = model["results"][None]
    assert rc == 0, out[-4000:]
    lines = out.strip().splitlines()
    words = lines[-1].split()
    runs = [l for l in lines if l.startswith("ok ") and " policy=" in l]
    assert words[0] == "ok" and int(words[1]) == len(runs) and int(words[2]) > 50000, lines[-1]
    scenarios = {l.split()[1] for l in runs}
    assert len(scenarios) >= 22 + N_RANDOM and len(runs) == 3 * len(scenarios)  # every scenario under none, all and random
    for must in ("steady_two_buffers_8200_channels", "refused_arguments", "changing_geometry_one_buffer", "pair_flags", "mixed_boundaries", "marks", "transcoding_chain",
                 "two_pipelines_share_the_streams", "random_%03d" % (N_RANDOM - 1)):
        assert must in scenarios, must


def test_every_mutant_is_rejected(model):
    """the kill table: which scenarios (and how many random programs) reject which mutant"""
    table, alive = [], []
    for name in MUTANTS:
        rc, out = model["results"][name]
        assert rc is not None, "%r does not link:\n%s" % (name, out[-2000:])
        failed = _failed_scenarios(out)
        if rc == 0 or (not failed and "Sanitizer" not in out):
            alive.append(name)
            continue
        scripted = sorted(s for s in failed if not s.startswith("random_"))
        n_random = sum(1 for s in failed if s.startswith("random_"))
        how = ", ".join(scripted) if scripted else ""
        if "Sanitizer" in out:  # (a mutant that reads past the caller's array ends the program there)
            how = (how + "; " if how else "") + "the sanitizer: " + next(l for l in out.splitlines() if "Sanitizer" in l).strip()[:120]
        first = next(iter(failed.values()))[0][1][:150] if failed else ""
        table.append("%-62s killed by %s%s\n%-62s   e.g. %s" % (name, how or "-", " + %d of %d random programs" % (n_random, N_RANDOM) if n_random else "", "", first))
    print("\n".join(["", "mutant kill table (%s build)" % ("sanitized" if model["sanitized"] else "UNSANITIZED")] + table))
    assert not alive, "mutants no scenario rejects: %s" % alive
