"""The upload ring of the companion libraries (lc3-codec_amd/csrc/lc3_host_ring.h) against fake HIP calls (tests/ring/lc3_ring_main.cpp),
on the CPU.

The ring is the only thing between a pinned slot that a call fills again and an earlier call's copy still in flight, and between two
kernels of one companion on two streams; a GPU test that compares results after a wait passes with either wait missing almost every time
(tests/test_pipeline_hb.py).  Here the header itself is compiled with g++ and linked with fakes of the twelve hip* functions it calls,
which execute nothing, log every call, count live allocations and events and fail on request; scripted scenarios assert over the log.  The
program has its own main, is built with -fsanitize=address,undefined (runtimes linked statically) and runs as a child process; nothing of
it is loaded into Python and no process of it opens a GPU.

A green run proves nothing by itself: the same program is also built from MUTANTS of the header -- one textual replacement each, applied
to a temporary copy, the replaced text asserted to occur exactly once -- and every mutant must be rejected."""
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lc3-codec_amd", "csrc")
RING_SRC = os.path.join(CSRC, "lc3_host_ring.h")
MAIN_SRC = os.path.join(ROOT, "tests", "ring", "lc3_ring_main.cpp")

# what the header calls, and the fakes therefore define: exactly these
HIP_CALLS = {"hipGetDevice", "hipSetDevice", "hipHostMalloc", "hipMalloc", "hipHostFree", "hipFree", "hipEventCreateWithFlags", "hipEventDestroy",
             "hipEventSynchronize", "hipEventRecord", "hipStreamWaitEvent", "hipGetLastError"}
SCENARIOS = ["no_early_wait", "cross_stream_ordered", "cross_stream_unordered", "acquire_without_commit", "commit_failing",
             "create_failing_at_each_step", "destroy", "device_guard"]

RECORD = "    const hipError_t e = hipEventRecord(r.done[k], stream);\n"
# name -> (the text replaced, which occurs exactly once; its replacement)
MUTANTS = {
    "the slot's event is not synchronised": ("    if (r.recorded[k]) {  // (returns at once", "    if (false) {  // (returns at once"),
    "no wait behind the previous call on another stream": ("if (ordered && r.last_slot >= 0 && r.last_stream != stream) {", "if (false) {"),
    "the stateless companions wait across streams too": ("if (ordered && r.last_slot >= 0 &&", "if (r.last_slot >= 0 &&"),
    "acquire advances next": ("    d_slot = r.d_ring + (size_t)k * r.slot_bytes;\n", "    d_slot = r.d_ring + (size_t)k * r.slot_bytes;\n    r.next = (k + 1) % kRingSlots;\n"),
    "recorded is marked before the record succeeds": (RECORD, "    r.recorded[k] = true;\n" + RECORD),
    "a failed create leaves its events behind": ("    if (e != hipSuccess) lc3_ring_destroy(r);\n", ""),
    "destroy waits for events that were never recorded": ("if (r.recorded[k]) (void)hipEventSynchronize(r.done[k]);", "(void)hipEventSynchronize(r.done[k]);"),
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
def ring():
    """{variant: (exit status, output)} for the header as it is (variant None) and for every mutant, and the hip* names the program of
    the header as it is refers to"""
    with open(RING_SRC) as f:
        text = f.read()
    sources = {None: text}
    for name, (old, new) in MUTANTS.items():
        assert text.count(old) == 1, "mutant %r: its text occurs %d times in lc3_host_ring.h" % (name, text.count(old))
        sources[name] = text.replace(old, new)
    inc = _rocm_include()
    base = ["g++", "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-result",
            "-Wno-deprecated-declarations"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    san_link = san + ["-static-libasan", "-static-libubsan"]  # (the program is whole, whatever else a machine loads into every process)
    jobs = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    with tempfile.TemporaryDirectory() as tmp:
        names = list(sources)
        dirs = {}
        for i, name in enumerate(names):
            dirs[name] = os.path.join(tmp, "v%02d" % i)
            os.makedirs(dirs[name])
            with open(os.path.join(dirs[name], "lc3_host_ring.h"), "w") as f:
                f.write(sources[name])
        # one probe decides whether this compiler can link the sanitizer runtimes; without them the scenarios still run, unsanitized
        probe = os.path.join(tmp, "probe.cpp")
        with open(probe, "w") as f:
            f.write("int main() { return 0; }\n")
        probe_run = _run(["g++"] + san_link + ["-o", os.path.join(tmp, "probe"), probe])
        sanitized = probe_run.returncode == 0
        flags = base + (san_link if sanitized else [])

        def build_and_run(name):
            d = dirs[name]
            r = _run(flags + ["-I" + d, "-c", "-o", os.path.join(d, "ring.o"), MAIN_SRC])
            if r.returncode == 0:
                r = _run(flags + ["-o", os.path.join(d, "ring"), os.path.join(d, "ring.o")])
            if r.returncode != 0:
                return None, r.stdout
            r = _run([os.path.join(d, "ring")])
            return r.returncode, r.stdout

        with ThreadPoolExecutor(max_workers=jobs) as pool:
            results = dict(zip(names, pool.map(build_and_run, names)))
        symbols = [ln.split() for ln in _run(["nm", os.path.join(dirs[None], "ring.o")]).stdout.splitlines()]
    return {"results": results, "defined": {s[-1] for s in symbols if len(s) == 3 and s[1] == "T" and s[2].startswith("hip")},
            "undefined": {s[-1] for s in symbols if len(s) == 2 and s[0] == "U" and s[1].startswith("hip")}, "called": set(re.findall(r"\b(hip[A-Z]\w*)\(", text)),
            "sanitized": sanitized, "probe": probe_run.stdout}


def test_the_program_ran_under_address_and_undefined_behaviour_sanitizers(ring):
    """where the compiler cannot link the sanitizer runtimes the scenarios still run, unsanitized, and this test says so in the report"""
    if not ring["sanitized"]:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + (ring["probe"].strip().splitlines() or ["?"])[-1])
    assert ring["results"][None][0] == 0


def test_the_header_is_host_only_and_names_no_companion():
    with open(RING_SRC) as f:
        text = f.read()
    assert "#include <hip/hip_runtime_api.h>" in text and "hip_runtime.h" not in text
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert sorted(includes) == ["cstddef", "cstdint", "hip/hip_runtime_api.h"], includes
    for word in ("__global__", "__device__", "__shared__", "hipLaunchKernelGGL", "<<<", "inspect", "analy", "mixer", "resampl", "meter", "lc3insp_",
                 "lc3ana_", "lc3mix_", "lc3rs_", "lc3mtr_", "lc3_iv_", "lc3_mx_", "lc3_rs_", "lc3_mt_"):
        assert word not in text, word
    # and it is the one place that holds the ring: the five units include it below their device code and keep no copy
    found = sorted(f for f in os.listdir(CSRC) if re.search(r"kRingSlots|struct OnDevice", open(os.path.join(CSRC, f)).read()))
    assert found == ["lc3_host_ring.h"], found
    for name, ordered in (("inspector", "false"), ("analyzer", "true"), ("mixer", "false"), ("resampler", "true"), ("meter", "true")):
        with open(os.path.join(CSRC, "lc3gpu_%s.hip" % name)) as f:
            hip = f.read()
        device, host = hip.split("// ---- host side ", 1)
        assert '#include "lc3_host_ring.h"' in host and "lc3_host_ring" not in device, name
        assert host.count("lc3_ring_acquire(p->ring, stream, %s, h_slot, d_slot)" % ordered) == 1 and host.count("lc3_ring_acquire(") == 1, name
        assert host.count("lc3_ring_commit(p->ring, stream)") == 1 and host.count("lc3_ring_create(p->ring, ") == 1, name
        assert host.count("lc3_ring_destroy(p->ring)") == 1, name
        for call in ("hipEventRecord", "hipEventSynchronize", "hipStreamWaitEvent", "hipEventCreateWithFlags", "hipHostMalloc"):
            assert call not in host, (name, call)


def test_the_fakes_define_exactly_what_the_header_calls(ring):
    assert ring["called"] == HIP_CALLS, sorted(ring["called"] ^ HIP_CALLS)
    assert ring["defined"] == HIP_CALLS and not ring["undefined"], (sorted(ring["defined"] ^ HIP_CALLS), sorted(ring["undefined"]))


def test_the_header_as_it_is_passes_every_scenario(ring):
    rc, out = ring["results"][None]
    assert rc == 0, out[-4000:]
    lines = out.strip().splitlines()
    assert lines[-1] == "ok %d scenarios" % len(SCENARIOS), lines[-1]
    assert [l.split()[1] for l in lines[:-1]] == SCENARIOS and all(l.startswith("ok ") for l in lines), out


def test_every_mutant_is_rejected(ring):
    """the kill table: which scenarios reject which mutant"""
    table, alive = [], []
    for name in MUTANTS:
        rc, out = ring["results"][name]
        assert rc is not None, "%r does not build:\n%s" % (name, out[-2000:])
        failed = {}
        for m in re.finditer(r"^FAIL (\S+): (.*)$", out, re.M):
            failed.setdefault(m.group(1), []).append(m.group(2))
        if rc == 0 or (not failed and "Sanitizer" not in out):
            alive.append(name)
            continue
        how = ", ".join(sorted(failed))
        if "Sanitizer" in out:
            how = (how + "; " if how else "") + "the sanitizer: " + next(l for l in out.splitlines() if "Sanitizer" in l).strip()[:120]
        first = next(iter(failed.values()))[0][:150] if failed else ""
        table.append("%-58s killed by %s\n%-58s   e.g. %s" % (name, how or "-", "", first))
    print("\n".join(["", "mutant kill table (%s build)" % ("sanitized" if ring["sanitized"] else "UNSANITIZED")] + table))
    assert not alive, "mutants no scenario rejects: %s" % alive
