"""ctypes binding of liblc3gpu.so and the Python mirror of the reference API.

Names, argument meaning and error behaviour follow the reference:
  Lc3Encoder.calc_working_buffer_lengths / new / encode_frame   (encoder/lc3_encoder.rs:117-209)
  Lc3Decoder.calc_working_buffer_lengths / new / decode_frame   (decoder/lc3_decoder.rs:181-244)
plus the batch entry points (`encode` / `decode`) that take DEVICE pointers
(e.g. torch tensors' data_ptr()) and a HIP stream.  No torch types cross the ABI.
"""
import ctypes
import enum
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
# LC3GPU_PROFILE=1 selects the diagnostic build with in-kernel stage stamps (never used for timing claims)
_PROFILE = os.environ.get("LC3GPU_PROFILE", "0") == "1"
# LC3GPU_LIB=<file name under lib/> selects another build of the same sources (compiler / tuning experiments, e.g. one made with
# LC3_HIPCC_EXTRA="-DLC3_RECON_WAVES=6"); the default is the one build() produces
_LIB = os.path.join(_HERE, "lib", os.environ.get("LC3GPU_LIB") or ("liblc3gpu_prof.so" if _PROFILE else "liblc3gpu.so"))
_SRC = os.path.join(_HERE, "csrc", "lc3gpu.hip")
# The companion libraries: device code of their own (one ordinary unit with one kernel each, csrc/lc3gpu_<name>.hip ->
# lib/liblc3gpu_<name>.so) beside whichever main library is built.  The main library links them (run path $ORIGIN) and holds their
# host-side entry points only (csrc/lc3gpu_<name>_api.cpp), so its own kernels are what they were.  name -> the sources that only this
# companion's unit sees, beside its .hip; a new companion is one entry here.
_COMPANIONS = {
    "inspector": (),
    "analyzer": ("lc3_host_analyze_views.h", "lc3_dev_dec_analyze.h"),
    "mixer": ("lc3_host_mix_views.h", "lc3_dev_mix.h"),
    "resampler": ("lc3_host_resample_views.h", "lc3_dev_resample.h", "lc3_resample_tables.h"),
    "meter": ("lc3_host_measure_views.h", "lc3_dev_level.h"),
}
# sources the companions share and no unit of the main library sees: the views' check and plan, the upload ring
_COMPANION_SHARED = ("lc3_host_inspect_views.h", "lc3_host_ring.h")
# host-only sources of the library on top of its own C ABI (the pipeline object, the companions' entry points): plain C++ beside the HIP
# translation units
_HOST_SRCS = [os.path.join(_HERE, "csrc", "lc3gpu_pipeline.cpp")] + [os.path.join(_HERE, "csrc", "lc3gpu_%s_api.cpp" % _n) for _n in _COMPANIONS]

class Lc3GpuError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = _strerror(code)
        super().__init__(f"lc3gpu error {code} ({msg}){': ' + what if what else ''}")


class Lc3EncoderError(Lc3GpuError):
    """The reference's Lc3EncoderError is an empty enum (lc3_encoder.rs:29-30): encode never returns Err.
    Raised here only where the reference panics (bad channel index / slice length)."""


class Lc3DecoderError(Lc3GpuError):
    """Lc3DecoderError::Only16BitsPerAudioSampleSupported (lc3_decoder.rs:36-42,80-82) and the panics."""


class SamplingFrequency(enum.IntEnum):  # common/config.rs:1-9
    Hz8000 = 8000
    Hz16000 = 16000
    Hz24000 = 24000
    Hz32000 = 32000
    Hz44100 = 44100
    Hz48000 = 48000


class FrameDuration(enum.IntEnum):  # common/config.rs:11-15 (microseconds)
    SevenPointFiveMs = 7500
    TenMs = 10000


_lib = None


def library_path():
    return _LIB


def companion_library_path(name):
    """the companion library of that name (a key of _COMPANIONS), which the main library links: beside the main library"""
    if name not in _COMPANIONS:
        raise KeyError(name)
    return os.path.join(os.path.dirname(_LIB), "liblc3gpu_%s.so" % name)


def inspector_library_path():
    """the companion library of the inspector (lc3gpu_inspect_mixed_views)"""
    return companion_library_path("inspector")


def analyzer_library_path():
    """the companion library of the analyzer (lc3gpu_analyze_mixed_views)"""
    return companion_library_path("analyzer")


def mixer_library_path():
    """the companion library of the mixer (lc3gpu_mix_mixed_views)"""
    return companion_library_path("mixer")


def resampler_library_path():
    """the companion library of the resampler (lc3gpu_resample_mixed_views)"""
    return companion_library_path("resampler")


def meter_library_path():
    """the companion library of the meter (lc3gpu_measure_mixed_views)"""
    return companion_library_path("meter")


def companion_own(name):
    """the file names of the sources that only this companion's unit sees: its .hip and its entry of the table"""
    return ("lc3gpu_%s.hip" % name,) + _COMPANIONS[name]


def _device_sources():
    """every source a HIP translation unit of any library could see: the headers and units under csrc/, the public header, the tables"""
    csrc = os.path.join(_HERE, "csrc")
    return [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip"))] + [
        os.path.join(_ROOT, "include", "lc3gpu.h"), os.path.join(_ROOT, "tables", "lc3_tables.h"), os.path.join(_ROOT, "tables", "lc3_resample_tables.h")]


def companion_sources(name):
    """the files a companion's stamp hashes -- what its unit can see: its own sources, the ones the companions share and the common device
    headers; none of another companion's own"""
    hidden = {f for other in _COMPANIONS if other != name for f in companion_own(other)}
    return [p_ for p_ in _device_sources() if os.path.basename(p_) not in hidden]


def main_sources():
    """the files the stamps of the main library's translation units hash: no companion's own sources and none of the shared ones"""
    hidden = {f for name in _COMPANIONS for f in companion_own(name)} | set(_COMPANION_SHARED)
    return [p_ for p_ in _device_sources() if os.path.basename(p_) not in hidden]


def _translation_units():
    """(kind, index) of every translation unit of the multi-unit build (csrc/lc3gpu.hip, "translation units"): the main unit (0: host
    side + the whole-source module's device code), the encoder kernels (1) and the decoder kernels (3) of every configuration view beyond
    the base ones, one unit per mixed-configuration kernel (2)"""
    import re

    with open(os.path.join(_HERE, "csrc", "lc3_cfg_views.h")) as f:
        text = f.read()
    n_all = int(re.search(r"#define LC3_N_VIEWS_ALL (\d+)", text).group(1))
    n_base = int(re.search(r"#define LC3_N_VIEWS_BASE (\d+)", text).group(1))
    return [(0, 0)] + [(k, v) for v in range(n_base + 1, n_all + 1) for k in (1, 3)] + [(2, k) for k in range(8)]


def _sources_hash(srcs):
    """sha256 over the CONTENTS of every source a library is built from.  Freshness is decided by content, not by time stamps: an object
    whose compile started before an edit and ended after it is newer than the sources and still stale (seen in round 5: a test session's
    build running while the sources were being edited left exactly that)"""
    import hashlib

    h = hashlib.sha256()
    for path in sorted(srcs):
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _build_signature(single, extra, extra_main, units, src_hash):
    """what a built library is a function of: the sources' contents and the build switches (advisor, round 4: switching LC3_SINGLE_TU /
    LC3_HIPCC_EXTRA used to leave a library of the other flavour in place)"""
    return "sources=%s single=%d extra=%s extra_main=%s units=%s profile=%d\n" % (
        src_hash, single, " ".join(extra), " ".join(extra_main), ",".join("%d_%d" % u for u in units), _PROFILE)


def build_native(force=False, verbose=False):
    """Compile csrc/lc3gpu.hip for gfx950 into lib/liblc3gpu.so (hipcc cross-compiles without a GPU).  The default library is built from
    several translation units of the same source side by side (device code generation is serial inside one unit; LC3_BUILD_JOBS, default
    the CPUs this process may use) and carries a compile-time view of every standard configuration; LC3_SINGLE_TU=1, the diagnostic build
    (LC3GPU_PROFILE=1) and builds with LC3_HIPCC_EXTRA compile it whole, with the four views of the round-1..4 library.
    LC3_HIPCC_EXTRA_MAIN="-D..." (timing experiments on the headline kernels): the multi-unit build with those flags on the MAIN unit only;
    the other units' objects are the production ones.  A library remembers the switches it was built with (<lib>.stamp) and is rebuilt
    when they differ; experiment builds need their own file name (LC3GPU_LIB) so that they never replace the default library.
    Every flavour links every companion library of the table (_COMPANIONS: csrc/lc3gpu_<name>.hip -> lib/liblc3gpu_<name>.so, one ordinary
    unit each), which are built and stamped here first, each with the sources its unit can see (companion_sources); their own and their
    shared sources are no part of what the main library's translation units are stamped with (main_sources)."""
    csrc = os.path.join(_HERE, "csrc")
    srcs = _device_sources() + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".cpp")]
    src_hash = _sources_hash(srcs)  # taken BEFORE anything is compiled: what the objects below are guaranteed to be at least as old as
    # (the HIP translation units do not see the host-only sources: an edit there relinks the library without recompiling them)
    dev_hash = _sources_hash(main_sources())
    extra = os.environ.get("LC3_HIPCC_EXTRA", "").split()  # compiler experiments
    extra_main = os.environ.get("LC3_HIPCC_EXTRA_MAIN", "").split()
    if (extra or extra_main) and not os.environ.get("LC3GPU_LIB"):
        raise RuntimeError("LC3_HIPCC_EXTRA / LC3_HIPCC_EXTRA_MAIN builds are experiments: name their library with LC3GPU_LIB=liblc3gpu_<what>.so")
    single = _PROFILE or bool(extra) or os.environ.get("LC3_SINGLE_TU", "0") == "1"
    units = [] if single else _translation_units()
    sig = _build_signature(single, extra, extra_main, units, src_hash)
    stamp = _LIB + ".stamp"

    def stamped(path, text):
        try:
            with open(path) as f:
                return f.read() == text
        except OSError:
            return False

    os.makedirs(os.path.dirname(_LIB), exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
             "-Wno-missing-braces"]
    # the companions first (every flavour of the main library links the same ones): one ordinary unit each, stamped with the contents of
    # the sources that unit can see (a companion's stamp does not change when another one is added: its sources are hidden from it)
    force_link = False
    for name in _COMPANIONS:
        comp_lib = companion_library_path(name)
        comp_sig = "sources=%s\n" % _sources_hash(companion_sources(name))
        if force or not os.path.exists(comp_lib) or not stamped(comp_lib + ".stamp", comp_sig):
            tmp = comp_lib + ".tmp%d" % os.getpid()
            cmd = ["hipcc"] + flags + ["-shared", "-o", tmp, os.path.join(csrc, "lc3gpu_%s.hip" % name)]
            if verbose:
                print(" ".join(cmd))
            try:
                subprocess.check_call(cmd)
                os.replace(tmp, comp_lib)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
            with open(comp_lib + ".stamp", "w") as f:
                f.write(comp_sig)
            force_link = True
    if not force and not force_link and os.path.exists(_LIB) and stamped(stamp, sig):
        return _LIB
    link_insp = ["-L" + os.path.dirname(_LIB)] + ["-llc3gpu_" + name for name in _COMPANIONS] + ["-Wl,-rpath,$ORIGIN"]
    if single:
        cmd = ["hipcc"] + extra + (["-DLC3_PROFILE"] if _PROFILE else []) + flags + ["-shared", "-o", _LIB, _SRC] + _HOST_SRCS + link_insp
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        with open(stamp, "w") as f:
            f.write(sig)
        return _LIB
    from concurrent.futures import ThreadPoolExecutor

    objdir = os.path.join(os.path.dirname(_LIB), "obj")
    os.makedirs(objdir, exist_ok=True)
    tag = os.path.splitext(os.path.basename(_LIB))[0]

    def unit_obj(u):  # an experiment's main unit gets an object of its own; every other object is shared with the production build
        return os.path.join(objdir, ("%s_0_0.o" % tag) if (extra_main and u == (0, 0)) else "lc3gpu_%d_%d.o" % u)

    def compile_unit(u):
        obj, tmp = unit_obj(u), unit_obj(u) + ".tmp%d" % os.getpid()
        cmd = ["hipcc", "-DLC3_TU_KIND=%d" % u[0], "-DLC3_TU_INDEX=%d" % u[1]] + (extra_main if u == (0, 0) else []) + flags + ["-c", "-o", tmp, _SRC]
        try:
            subprocess.check_call(cmd)
            os.replace(tmp, obj)  # (a unit that fails leaves no partial object behind)
            with open(obj + ".stamp", "w") as f:
                f.write(unit_sig(u))
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        return obj

    def unit_sig(u):
        return "sources=%s flags=%s\n" % (dev_hash, " ".join(extra_main) if u == (0, 0) else "")

    def fresh(u):
        o = unit_obj(u)
        return os.path.exists(o) and stamped(o + ".stamp", unit_sig(u))

    try:
        jobs = len(os.sched_getaffinity(0))
    except AttributeError:
        jobs = os.cpu_count() or 1
    jobs = max(1, int(os.environ.get("LC3_BUILD_JOBS", jobs)))
    # (the main unit and the mixed-kernel units are the long ones: first).  Objects stamped with these sources' hash are kept unless forced;
    # an experiment build never recompiles the shared ones it finds up to date
    order = sorted(units, key=lambda u: (u[0] != 0, u[0] != 2))
    todo = [u for u in order if (force and (not extra_main or u == (0, 0))) or not fresh(u)]
    if verbose:
        print("hipcc -DLC3_TU_KIND=k -DLC3_TU_INDEX=i %s -c %s   x %d of %d translation units, %d at a time" % (
            " ".join(flags), _SRC, len(todo), len(units), jobs))
    with ThreadPoolExecutor(max_workers=jobs) as pool:
        list(pool.map(compile_unit, todo))
    host_objs = []
    for src in _HOST_SRCS:  # (seconds each: always recompiled)
        obj = os.path.join(objdir, os.path.splitext(os.path.basename(src))[0] + ".o")
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", "-fPIC", "-c", "-o", obj, src])
        host_objs.append(obj)
    cmd = ["hipcc", "--offload-arch=gfx950", "-fPIC", "-shared", "-o", _LIB] + sorted(unit_obj(u) for u in units) + host_objs + link_insp
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(sig)
    return _LIB


def tool_path():
    return os.path.join(os.path.dirname(_LIB), "lc3gpu-tool")


def build_tool(force=False, verbose=False):
    """Compile the file-driver command line tool (host/lc3_files.cpp, host/lc3gpu_tool.cpp) against liblc3gpu.so."""
    host = os.path.join(_HERE, "host")
    srcs = [os.path.join(host, f) for f in ("lc3_files.cpp", "lc3gpu_tool.cpp")]
    deps = srcs + [os.path.join(host, "lc3_files.hpp"), os.path.join(_ROOT, "include", "lc3gpu.h"),
                   os.path.join(_ROOT, "include", "lc3gpu.hpp"), _LIB]
    out = tool_path()
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    cmd = ["hipcc", "-O2", "-std=c++17", "-Wno-unused-result", "-o", out] + srcs + [
        "-L" + os.path.dirname(_LIB), "-llc3gpu", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def load_library():
    """Load liblc3gpu.so; fails loudly if the native extension is missing (there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64
    # under torch/lib.  If the system runtime (/opt/rocm) is mapped first through this library, a later
    # `import torch` binds to the wrong runtime and torch.cuda reports no device.  When torch is installed
    # (it is only used by callers for device memory / streams), let it bring in its runtime first.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional for the C ABI
        pass
    if not os.path.exists(_LIB):
        raise ImportError(f"{_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the LC3 engine has no non-native path)")
    L = ctypes.CDLL(_LIB)
    vp, i, pi64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)
    L.lc3gpu_strerror.restype = ctypes.c_char_p
    L.lc3gpu_strerror.argtypes = [i]
    L.lc3gpu_config.argtypes = [i, i, vp]
    L.lc3gpu_encoder_working_buffer_lengths.argtypes = [i, i, i, pi64]
    L.lc3gpu_decoder_working_buffer_lengths.argtypes = [i, i, i, pi64]
    L.lc3gpu_encoder_create.argtypes = [ctypes.POINTER(vp), i, i, i]
    L.lc3gpu_encoder_create_spec.argtypes = [ctypes.POINTER(vp), i, i, i, i]
    L.lc3gpu_encoder_create_mixed_spec.argtypes = [ctypes.POINTER(vp), i, vp, i]
    L.lc3gpu_encoder_destroy.argtypes = [vp]
    L.lc3gpu_encoder_reset.argtypes = [vp]
    L.lc3gpu_encode_frame.argtypes = [vp, i, vp, i, vp, i]
    L.lc3gpu_encode_frame_debug.argtypes = [vp, vp, i, vp, i, vp]
    L.lc3gpu_encode.argtypes = [vp, vp, vp, i, i, vp]
    L.lc3gpu_encode_range.argtypes = [vp, i, i, vp, vp, i, i, vp]
    L.lc3gpu_encode_vbr.argtypes = [vp, vp, vp, vp, i, i, vp]
    L.lc3gpu_encode_list.argtypes = [vp, vp, i, vp, vp, i, i, vp]
    L.lc3gpu_decode_list.argtypes = [vp, vp, i, vp, vp, vp, i, i, vp]
    L.lc3gpu_encode_mixed_list.argtypes = [vp, vp, i, vp, vp, i, vp]
    L.lc3gpu_decode_mixed_list.argtypes = [vp, vp, i, vp, vp, vp, i, vp]
    L.lc3gpu_encode_mixed_items.argtypes = [vp, vp, i, vp, vp, vp]
    L.lc3gpu_decode_mixed_items.argtypes = [vp, vp, i, vp, vp, vp, vp]
    L.lc3gpu_encode_mixed_mc_items.argtypes = [vp, vp, i, vp, vp, vp]
    L.lc3gpu_decode_mixed_mc_items.argtypes = [vp, vp, i, vp, vp, vp, vp]
    L.lc3gpu_encode_mixed_views.argtypes = [vp, vp, i, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    L.lc3gpu_decode_mixed_views.argtypes = [vp, vp, i, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    L.lc3gpu_encoder_reset_channels.argtypes = [vp, vp, i]
    L.lc3gpu_decoder_reset_channels.argtypes = [vp, vp, i]
    L.lc3gpu_encoder_state_save_channels.argtypes = [vp, vp, i, vp, ctypes.c_size_t]
    L.lc3gpu_encoder_state_load_channels.argtypes = [vp, vp, i, vp, ctypes.c_size_t]
    L.lc3gpu_decoder_state_save_channels.argtypes = [vp, vp, i, vp, ctypes.c_size_t]
    L.lc3gpu_decoder_state_load_channels.argtypes = [vp, vp, i, vp, ctypes.c_size_t]
    L.lc3gpu_encoder_size_clamps.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.lc3gpu_decode_vbr.argtypes = [vp, vp, vp, vp, vp, i, i, vp]
    L.lc3gpu_inspect.argtypes = [i, i, vp, vp, vp, i, i, vp, vp]
    L.lc3gpu_inspector_create.argtypes = [ctypes.POINTER(vp), i, vp, i]
    L.lc3gpu_inspector_destroy.argtypes = [vp]
    L.lc3gpu_inspect_mixed_views.argtypes = [vp, vp, i, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    L.lc3gpu_analyzer_create.argtypes = [ctypes.POINTER(vp), i, vp, i, i]
    L.lc3gpu_analyzer_destroy.argtypes = [vp]
    L.lc3gpu_analyze_mixed_views.argtypes = [vp, vp, i, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp,
                                             ctypes.c_size_t, vp]
    L.lc3gpu_mixer_create.argtypes = [ctypes.POINTER(vp), i, vp, i]
    L.lc3gpu_mixer_destroy.argtypes = [vp]
    L.lc3gpu_mix_mixed_views.argtypes = [vp, vp, vp, i, vp, ctypes.c_size_t, vp, vp, i, vp, ctypes.c_size_t, vp]
    L.lc3gpu_resampler_create.argtypes = [ctypes.POINTER(vp), i, vp, i]
    L.lc3gpu_resampler_destroy.argtypes = [vp]
    L.lc3gpu_resampler_reset.argtypes = [vp]
    L.lc3gpu_resampler_reset_channels.argtypes = [vp, vp, i]
    L.lc3gpu_resample_mixed_views.argtypes = [vp, vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_size_t, i, vp]
    L.lc3gpu_meter_create.argtypes = [ctypes.POINTER(vp), i, vp, i]
    L.lc3gpu_meter_destroy.argtypes = [vp]
    L.lc3gpu_meter_reset.argtypes = [vp]
    L.lc3gpu_meter_reset_channels.argtypes = [vp, vp, i]
    L.lc3gpu_measure_mixed_views.argtypes = [vp, vp, i, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    L.lc3gpu_encoder_state_size.restype = ctypes.c_size_t
    L.lc3gpu_encoder_state_size.argtypes = [vp]
    L.lc3gpu_encoder_state_save.argtypes = [vp, vp, ctypes.c_size_t]
    L.lc3gpu_encoder_state_load.argtypes = [vp, vp, ctypes.c_size_t]
    L.lc3gpu_encode_layout.argtypes = [vp, i, vp, vp, i, i, vp]
    L.lc3gpu_encoder_create_mixed.argtypes = [ctypes.POINTER(vp), i, vp]
    L.lc3gpu_encode_mixed.argtypes = [vp, vp, vp, i, vp]
    L.lc3gpu_decoder_create.argtypes = [ctypes.POINTER(vp), i, i, i]
    L.lc3gpu_decoder_destroy.argtypes = [vp]
    L.lc3gpu_decoder_reset.argtypes = [vp]
    L.lc3gpu_decode_frame.argtypes = [vp, i, i, vp, i, vp, i]
    L.lc3gpu_decode.argtypes = [vp, vp, vp, vp, i, i, vp]
    L.lc3gpu_decode_range.argtypes = [vp, i, i, vp, vp, vp, i, i, vp]
    L.lc3gpu_decoder_state_size.restype = ctypes.c_size_t
    L.lc3gpu_decoder_state_size.argtypes = [vp]
    L.lc3gpu_decoder_state_save.argtypes = [vp, vp, ctypes.c_size_t]
    L.lc3gpu_decoder_state_load.argtypes = [vp, vp, ctypes.c_size_t]
    L.lc3gpu_decode_layout.argtypes = [vp, i, vp, vp, vp, i, i, vp]
    L.lc3gpu_decoder_create_mixed.argtypes = [ctypes.POINTER(vp), i, vp]
    L.lc3gpu_decode_mixed.argtypes = [vp, vp, vp, vp, i, vp]
    L.lc3gpu_decoder_plc_events.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.lc3gpu_encoder_pair_timeouts.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.lc3gpu_decoder_pair_timeouts.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.lc3gpu_kernel_info.argtypes = [i, vp]
    L.lc3gpu_encoder_timing.argtypes = [vp, i, vp]
    L.lc3gpu_decoder_timing.argtypes = [vp, i, vp]
    L.lc3gpu_decoder_timing_kernels.argtypes = [vp, i, vp]
    L.lc3gpu_decode_frame_debug.argtypes = [vp, i, vp, i, vp, i, vp]
    L.lc3gpu_decoder_synth_debug.argtypes = [vp, i, vp, i, i, i, i, vp, i, vp]
    L.lc3gpu_selftest_math.argtypes = [i, vp, vp, i, vp]
    L.lc3gpu_clock_probe.argtypes = [vp, vp, i]
    L.lc3gpu_encoder_stage_event.argtypes = [vp, i, vp]
    L.lc3gpu_decoder_stage_event.argtypes = [vp, i, vp]
    L.lc3gpu_encoder_bind_stream.argtypes = [vp, vp, i]
    L.lc3gpu_decoder_bind_stream.argtypes = [vp, vp, i]
    L.lc3gpu_encoder_debug_pair_giveup.argtypes = [vp]
    L.lc3gpu_decoder_debug_pair_giveup.argtypes = [vp]
    L.lc3gpu_encoder_pair_pending.argtypes = [vp]
    L.lc3gpu_decoder_pair_pending.argtypes = [vp]
    L.lc3gpu_encode_host.argtypes = [vp, vp, vp, i, i]
    L.lc3gpu_decode_host.argtypes = [vp, vp, vp, vp, i, i]
    L.lc3gpu_host_alloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    L.lc3gpu_host_free.argtypes = [vp]
    L.lc3gpu_pipeline_create.argtypes = [ctypes.POINTER(vp), i, i, i, i]
    L.lc3gpu_pipeline_create_mixed.argtypes = [ctypes.POINTER(vp), i, vp, i, vp]
    L.lc3gpu_pipeline_submit_mixed.argtypes = [vp, vp, vp, vp, i]
    L.lc3gpu_pipeline_encode_mixed.argtypes = [vp, vp, vp, i]
    L.lc3gpu_pipeline_decode_mixed.argtypes = [vp, vp, vp, vp, i]
    L.lc3gpu_pipeline_destroy.argtypes = [vp]
    L.lc3gpu_pipeline_reset.argtypes = [vp]
    L.lc3gpu_pipeline_submit.argtypes = [vp, vp, vp, vp, i, i]
    L.lc3gpu_pipeline_encode.argtypes = [vp, vp, vp, i, i]
    L.lc3gpu_pipeline_decode.argtypes = [vp, vp, vp, vp, i, i]
    L.lc3gpu_pipeline_wait.argtypes = [vp]
    L.lc3gpu_pipeline_join.argtypes = [vp, vp]
    L.lc3gpu_pipeline_follow.argtypes = [vp, vp]
    L.lc3gpu_pipeline_mark.argtypes = [vp, vp]
    L.lc3gpu_pipeline_groups.argtypes = [vp]
    L.lc3gpu_pipeline_group.argtypes = [vp, i, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.lc3gpu_pipeline_last_hip_error.argtypes = [vp]
    _lib = L
    return L


# every symbol include/lc3gpu.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "lc3gpu_version", "lc3gpu_strerror", "lc3gpu_last_hip_error", "lc3gpu_device_count", "lc3gpu_config",
    "lc3gpu_encoder_working_buffer_lengths", "lc3gpu_decoder_working_buffer_lengths", "lc3gpu_encoder_create",
    "lc3gpu_encoder_destroy", "lc3gpu_encoder_reset", "lc3gpu_encode_frame", "lc3gpu_encode", "lc3gpu_encode_range",
    "lc3gpu_encoder_state_size", "lc3gpu_encoder_state_save", "lc3gpu_encoder_state_load", "lc3gpu_decoder_create",
    "lc3gpu_decoder_destroy", "lc3gpu_decoder_reset", "lc3gpu_decode_frame", "lc3gpu_decode", "lc3gpu_decode_range",
    "lc3gpu_decoder_state_size", "lc3gpu_decoder_state_save", "lc3gpu_decoder_state_load",
    "lc3gpu_decoder_plc_events", "lc3gpu_encode_frame_debug", "lc3gpu_kernel_info", "lc3gpu_prof_read", "lc3gpu_encoder_timing", "lc3gpu_decoder_timing",
    "lc3gpu_decoder_timing_kernels", "lc3gpu_decode_frame_debug", "lc3gpu_decoder_synth_debug", "lc3gpu_selftest_math", "lc3gpu_encode_layout", "lc3gpu_decode_layout", "lc3gpu_encoder_create_mixed", "lc3gpu_decoder_create_mixed", "lc3gpu_encode_mixed",
    "lc3gpu_decode_mixed", "lc3gpu_encoder_create_spec", "lc3gpu_encoder_create_mixed_spec", "lc3gpu_clock_probe",
    "lc3gpu_encoder_stage_event", "lc3gpu_decoder_stage_event", "lc3gpu_encoder_pair_timeouts", "lc3gpu_decoder_pair_timeouts",
    "lc3gpu_encoder_debug_pair_giveup", "lc3gpu_decoder_debug_pair_giveup", "lc3gpu_encoder_pair_pending", "lc3gpu_decoder_pair_pending", "lc3gpu_encoder_bind_stream", "lc3gpu_decoder_bind_stream", "lc3gpu_encode_host", "lc3gpu_decode_host", "lc3gpu_host_alloc",
    "lc3gpu_host_free", "lc3gpu_pipeline_create", "lc3gpu_pipeline_create_mixed", "lc3gpu_pipeline_submit_mixed", "lc3gpu_pipeline_encode_mixed",
    "lc3gpu_pipeline_decode_mixed", "lc3gpu_pipeline_destroy", "lc3gpu_pipeline_reset", "lc3gpu_pipeline_submit",
    "lc3gpu_pipeline_encode", "lc3gpu_pipeline_decode", "lc3gpu_pipeline_wait", "lc3gpu_pipeline_join", "lc3gpu_pipeline_follow", "lc3gpu_pipeline_mark",
    "lc3gpu_pipeline_groups", "lc3gpu_pipeline_group", "lc3gpu_pipeline_last_hip_error", "lc3gpu_encode_vbr", "lc3gpu_encoder_size_clamps", "lc3gpu_decode_vbr",
    "lc3gpu_inspect", "lc3gpu_encode_list", "lc3gpu_decode_list", "lc3gpu_encoder_reset_channels", "lc3gpu_decoder_reset_channels",
    "lc3gpu_encoder_state_save_channels", "lc3gpu_encoder_state_load_channels", "lc3gpu_decoder_state_save_channels",
    "lc3gpu_decoder_state_load_channels", "lc3gpu_encode_mixed_list", "lc3gpu_decode_mixed_list",
    "lc3gpu_encode_mixed_items", "lc3gpu_decode_mixed_items",
    "lc3gpu_encode_mixed_mc_items", "lc3gpu_decode_mixed_mc_items",
    "lc3gpu_encode_mixed_views", "lc3gpu_decode_mixed_views",
    "lc3gpu_inspector_create", "lc3gpu_inspector_destroy", "lc3gpu_inspect_mixed_views",
    "lc3gpu_analyzer_create", "lc3gpu_analyzer_destroy", "lc3gpu_analyze_mixed_views",
    "lc3gpu_mixer_create", "lc3gpu_mixer_destroy", "lc3gpu_mix_mixed_views",
    "lc3gpu_resampler_create", "lc3gpu_resampler_destroy", "lc3gpu_resampler_reset", "lc3gpu_resampler_reset_channels",
    "lc3gpu_resample_mixed_views",
    "lc3gpu_meter_create", "lc3gpu_meter_destroy", "lc3gpu_meter_reset", "lc3gpu_meter_reset_channels", "lc3gpu_measure_mixed_views",
]

# LC3GPU_SPEC_*: opt-in corrections of the reference's deviations from the LC3 specification (default 0 = reference behaviour)
SPEC_8KHZ_ENCODE, SPEC_TNS_SSWB_STOP, SPEC_BW_CUTOFF_DB, SPEC_SNS_LAST_GAIN, SPEC_NBITS_SPEC_OLD, SPEC_ALL = 1, 2, 4, 8, 16, 31

LAYOUT_PLANAR, LAYOUT_INTERLEAVED = 0, 1
# stage events (LC3GPU_ENC_STAGE_* / LC3GPU_DEC_STAGE_*)
ENC_STAGE_FRONT, ENC_STAGE_VQ, ENC_STAGE_BACK, DEC_STAGE_PARSE = 0, 1, 2, 0


# frame inspection (lc3gpu_inspect): the record of one frame (lc3gpu_frame_info, 128 bytes) and its status codes (LC3GPU_FRAME_*)
FRAME_INFO_DTYPE = np.dtype([
    ("status", "<i4"), ("nbytes", "<i4"),
    ("bandwidth", "<i4"), ("lastnz", "<i4"), ("lsb_mode", "<i4"), ("global_gain_index", "<i4"), ("num_tns_filters", "<i4"),
    ("rc_order_ari_input", "<i4", (2,)), ("sns_ind_lf", "<i4"), ("sns_ind_hf", "<i4"), ("sns_ls_inda", "<i4"), ("sns_ls_indb", "<i4"),
    ("sns_idx_a", "<u4"), ("sns_idx_b", "<u4"), ("sns_submode_lsb", "<i4"), ("sns_submode_msb", "<i4"), ("sns_g_ind", "<i4"),
    ("pitch_present", "<i4"), ("ltpf_active", "<i4"), ("pitch_index", "<i4"), ("noise_factor", "<i4"),
    ("rc_order", "<i4", (2,)), ("n_residual_bits", "<i4"), ("noise_filling_seed", "<i4"), ("is_zero_frame", "<i4"),
    ("rc_i", "u1", (16,)), ("reserved", "<i4"),
])
assert FRAME_INFO_DTYPE.itemsize == 128
FRAME_OK, FRAME_FLAGGED, FRAME_EMPTY, FRAME_SIDE_INFO, FRAME_ARITH = 0, 1, 2, 16, 32
# the reference's error of a frame (decoder/lc3_decoder.rs:36-42): Lc3DecoderError::SideInfo(SideInfoError::..) for FRAME_SIDE_INFO + k,
# Lc3DecoderError::ArithmeticDecode(ArithmeticDecodeError::..) for FRAME_ARITH + k
FRAME_STATUS_NAMES = {FRAME_OK: "Ok", FRAME_FLAGGED: "Flagged", FRAME_EMPTY: "Empty"}
for _k, _n in enumerate(("BufferReaderError", "BandwidthIdxOutOfRange", "LastNonZeroTupleGreaterThanYLen", "PlcTriggerSns1OutOfRange",
                         "PlcTriggerSns2OutOfRange"), 1):
    FRAME_STATUS_NAMES[FRAME_SIDE_INFO + _k] = "SideInfo::" + _n
for _k, _n in enumerate(("ArithmeticCodec", "TnsOrder", "TnsCoef", "SpectralData", "SpectralBoolData", "NegativeResidualNumBits", "ResidualBoolData",
                         "ResidualBoolDataOverflow"), 1):
    FRAME_STATUS_NAMES[FRAME_ARITH + _k] = "ArithmeticDecode::" + _n


def frame_status_name(status):
    return FRAME_STATUS_NAMES.get(int(status), "Unknown(%d)" % int(status))


def inspect(frame_duration, sampling_frequency, d_in, d_info, slot_bytes, n_frames, d_nbytes=None, d_bad_frame=None, stream=None):
    """lc3gpu_inspect: the side information and decode status of n_frames frames (include/lc3gpu.h).  DEVICE pointers (or tensors):
    d_in uint8[n_frames][slot_bytes], d_info FRAME_INFO_DTYPE[n_frames] (128 bytes per frame), d_nbytes uint16[n_frames] or None,
    d_bad_frame uint8[n_frames] or None.  Asynchronous on `stream`; needs no codec handle."""
    rc = load_library().lc3gpu_inspect(int(frame_duration), int(sampling_frequency), _ptr(d_in), _ptr(d_nbytes), _ptr(d_bad_frame),
                                       int(slot_bytes), int(n_frames), _ptr(d_info), _ptr(stream))
    if rc:
        raise Lc3GpuError(rc, "inspect")


def _event_handle(event):
    """a hipEvent_t as an integer: None, an integer, or an object with `cuda_event` (torch.cuda.Event -- record it once before passing it:
    torch creates the HIP event lazily)"""
    if event is None:
        return None
    h = getattr(event, "cuda_event", event)
    if not h:
        raise ValueError("the event has no HIP handle yet (torch.cuda.Event: record it once first)")
    return ctypes.c_void_p(int(h))
# stage dumps of Lc3Decoder.decode_frame_debug / synth_debug (LC3GPU_DBG_*)
DBG_INT, DBG_SPEC, DBG_IMDCT, DBG_LTPF, DBG_GAIN, DBG_TNS, DBG_FLOATS = 0, 400, 800, 1280, 1760, 2160, 2560
RECON_LANE, RECON_LATE, RECON_WAVE = 0, 1, 2
# stage dumps of Lc3Encoder.encode_frame_debug (LC3GPU_ENC_DBG_*)
ENC_DBG_SCALARS, ENC_DBG_EB, ENC_DBG_ATTACK, ENC_DBG_FLOATS = 1440, 1472, 1536, 1600


class StreamDesc(ctypes.Structure):
    """lc3gpu_stream_desc: one stream of a mixed-configuration handle"""
    _fields_ = [("fs_hz", ctypes.c_int), ("frame_us", ctypes.c_int), ("nbytes", ctypes.c_int)]


def _desc_array(descs):
    arr = (StreamDesc * len(descs))()
    for k, d in enumerate(descs):
        arr[k].fs_hz, arr[k].frame_us, arr[k].nbytes = int(d[0]), int(d[1]), int(d[2])
    return arr


def _layout(layout):
    if layout in (LAYOUT_PLANAR, "planar", None):
        return LAYOUT_PLANAR
    if layout in (LAYOUT_INTERLEAVED, "interleaved"):
        return LAYOUT_INTERLEAVED
    raise ValueError("layout must be 'planar' or 'interleaved'")



def _strerror(code):
    try:
        return load_library().lc3gpu_strerror(int(code)).decode()
    except Exception:
        return "?"


def selftest_math(which, x=None, d=None, n=None):
    """tests only: a float routine evaluated on the device (lc3gpu_selftest_math) -> float32[n]"""
    L = load_library()
    if x is not None:
        x = np.ascontiguousarray(x, np.float32)
        n = x.size
    if d is not None:
        d = np.ascontiguousarray(d, np.float32)
    out = np.zeros(int(n), np.float32)
    rc = L.lc3gpu_selftest_math(int(which), _ptr(x), _ptr(d), int(n), _ptr(out))
    if rc:
        raise Lc3GpuError(rc, "selftest_math")
    return out


def clock_probe(d_out, stream=None, spin=50000):
    """measurement aid: a one-wave kernel on `stream` leaves {shader cycles, 100 MHz ticks} of its spin in d_out (device uint64[3]);
    asynchronous.  clock = 100 MHz x cycles / ticks"""
    rc = load_library().lc3gpu_clock_probe(_ptr(stream), _ptr(d_out), int(spin))
    if rc:
        raise Lc3GpuError(rc, "clock_probe")


def device_count():
    return int(load_library().lc3gpu_device_count())


def _ptr(x):
    """device pointer (int) or host numpy array -> c_void_p"""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(ctypes.c_void_p)
    if hasattr(x, "data_ptr"):
        return ctypes.c_void_p(x.data_ptr())
    return ctypes.c_void_p(int(x))


def _channel_list(channels):
    """any integer sequence or numpy array -> contiguous HOST int32 array (the channel list of the *_list / *_channels calls)"""
    a = np.asarray(channels)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError("channel indices must be integers")
    return np.ascontiguousarray(a.reshape(-1), dtype=np.int32)


def _item_list(items):
    """a sequence of (channel, n_frames[, nbytes]) or an integer array [n][2..4] -> contiguous HOST int32[n][4], the lc3gpu_item array of
    the *_mixed_items calls (nbytes 0 = the descriptor's; the fourth word is reserved, 0 unless the caller's array sets it)"""
    rows = [tuple(r) for r in items]
    out = np.zeros((len(rows), 4), np.int32)
    for i, r in enumerate(rows):
        if not 2 <= len(r) <= 4:
            raise TypeError("an item is (channel, n_frames[, nbytes])")
        for v in r:
            if not isinstance(v, (int, np.integer)):
                raise TypeError("item fields must be integers")
        out[i, : len(r)] = r
    return out


def _mc_item_list(items):
    """a sequence of (first_channel, n_channels, n_frames[, nbytes]) or an integer array [n][3..4] -> contiguous HOST int32[n][4], the
    lc3gpu_mc_item array of the *_mixed_mc_items calls (nbytes 0 = the descriptors')"""
    rows = [tuple(r) for r in items]
    out = np.zeros((len(rows), 4), np.int32)
    for i, r in enumerate(rows):
        if not 3 <= len(r) <= 4:
            raise TypeError("an mc item is (first_channel, n_channels, n_frames[, nbytes])")
        for v in r:
            if not isinstance(v, (int, np.integer)):
                raise TypeError("item fields must be integers")
        out[i, : len(r)] = r
    return out


# lc3gpu_view (include/lc3gpu.h), 64 bytes: an item of the *_mixed_views calls with its own placement
VIEW_FIELDS = ("channel", "n_frames", "nbytes", "pcm_stride", "pcm_off", "byte_off", "flag_off", "pcm_pitch", "byte_pitch", "flag_pitch")
VIEW_DTYPE = np.dtype({"names": list(VIEW_FIELDS) + ["reserved"],
                       "formats": [np.int32] * 4 + [np.int64] * 3 + [np.int32] * 3 + [(np.int32, 3)],
                       "offsets": [0, 4, 8, 12, 16, 24, 32, 40, 44, 48, 52], "itemsize": 64})


def _view_list(views):
    """a sequence of tuples (channel, n_frames, nbytes, pcm_stride, pcm_off, byte_off[, flag_off[, pcm_pitch[, byte_pitch[, flag_pitch]]]])
    or of dicts over VIEW_FIELDS (channel, n_frames, pcm_off and byte_off required; pcm_stride defaults to 1, everything else to 0), or
    a VIEW_DTYPE array -> contiguous HOST VIEW_DTYPE[n], the lc3gpu_view array of the *_mixed_views calls"""
    if isinstance(views, np.ndarray) and views.dtype == VIEW_DTYPE:
        return np.ascontiguousarray(views.reshape(-1))
    rows = list(views)
    out = np.zeros(len(rows), VIEW_DTYPE)
    for i, r in enumerate(rows):
        if isinstance(r, dict):
            unknown = set(r) - set(VIEW_FIELDS)
            missing = {"channel", "n_frames", "pcm_off", "byte_off"} - set(r)
            if unknown or missing:
                raise TypeError("a view names %s and may name %s" % ("channel, n_frames, pcm_off, byte_off", ", ".join(VIEW_FIELDS)))
            r = dict({"pcm_stride": 1}, **r)
        else:
            r = tuple(r)
            if not 6 <= len(r) <= len(VIEW_FIELDS):
                raise TypeError("a view is (channel, n_frames, nbytes, pcm_stride, pcm_off, byte_off[, flag_off[, pcm_pitch[, byte_pitch[, flag_pitch]]]])")
            r = dict(zip(VIEW_FIELDS, r))
        for name, v in r.items():
            if not isinstance(v, (int, np.integer)):
                raise TypeError("view fields must be integers")
            out[i][name] = v
    return out


def _numel(x, what):
    """elements of a torch tensor or numpy array (the buffer extents the *_mixed_views calls check every view against)"""
    if hasattr(x, "numel"):
        return int(x.numel())
    if isinstance(x, np.ndarray):
        return int(x.size)
    raise TypeError("%s: pass the buffer's extent when the buffer is a bare pointer" % what)


def _records(buf, given, record_bytes, what):
    """the extent of an output in records of record_bytes: 0 without the output, else `given`, else from the size in bytes of the torch
    tensor or numpy array (whatever its element type); a bare pointer needs it given"""
    if buf is None:
        return 0
    if given is not None:
        return int(given)
    if isinstance(buf, np.ndarray) or hasattr(buf, "element_size"):
        size = buf.itemsize if isinstance(buf, np.ndarray) else buf.element_size()
        return _numel(buf, what) * int(size) // record_bytes
    raise TypeError("%s: pass the buffer's extent when the buffer is a bare pointer" % what)


class Lc3Config:
    """common/config.rs:18-100"""

    def __init__(self, sampling_frequency, frame_duration):
        out = (ctypes.c_int * 7)()
        rc = load_library().lc3gpu_config(int(frame_duration), int(sampling_frequency), out)
        if rc:
            raise Lc3GpuError(rc, "Lc3Config")
        self.fs_ind, self.fs, self.ne, n10, self.nb, self.nf, self.z = list(out)
        self.n_ms = FrameDuration.TenMs if n10 else FrameDuration.SevenPointFiveMs


class Lc3Encoder:
    """`num_channels` independent encoder channels resident on the current HIP device."""

    @staticmethod
    def calc_working_buffer_lengths(num_channels, frame_duration, sampling_frequency):
        """-> (integer_len, scaler_len, complex_len), lc3_encoder.rs:194-209"""
        out = (ctypes.c_int64 * 3)()
        rc = load_library().lc3gpu_encoder_working_buffer_lengths(num_channels, int(frame_duration),
                                                                  int(sampling_frequency), out)
        if rc:
            raise Lc3EncoderError(rc)
        return tuple(int(v) for v in out)

    def __init__(self, num_channels, frame_duration, sampling_frequency, spec_flags=0):
        self._L = load_library()
        self.config = Lc3Config(sampling_frequency, frame_duration)
        self.num_channels = int(num_channels)
        h = ctypes.c_void_p()
        rc = self._L.lc3gpu_encoder_create_spec(ctypes.byref(h), self.num_channels, int(frame_duration),
                                                int(sampling_frequency), int(spec_flags))
        if rc:
            raise Lc3EncoderError(rc, "Lc3Encoder::new")
        self._h = h

    new = classmethod(lambda cls, *a, **k: cls(*a, **k))

    @classmethod
    def mixed(cls, descs, spec_flags=0):
        """one handle for streams of different configurations: descs = [(fs_hz, frame_us, nbytes), ...] (lc3gpu_encoder_create_mixed)"""
        self = cls.__new__(cls)
        self._L = load_library()
        self.descs = [(int(d[0]), int(d[1]), int(d[2])) for d in descs]
        self.configs = [Lc3Config(d[0], d[1]) for d in self.descs]
        self.config = None
        self.num_channels = len(self.descs)
        h = ctypes.c_void_p()
        rc = self._L.lc3gpu_encoder_create_mixed_spec(ctypes.byref(h), self.num_channels, _desc_array(self.descs), int(spec_flags))
        if rc:
            raise Lc3EncoderError(rc, "Lc3Encoder::mixed")
        self._h = h
        return self

    def encode_mixed(self, d_pcm, d_out, n_frames, stream=None):
        """ragged DEVICE buffers, streams in descriptor order (include/lc3gpu.h); one launch per kernel"""
        rc = self._L.lc3gpu_encode_mixed(self._h, _ptr(d_pcm), _ptr(d_out), int(n_frames), _ptr(stream))
        if rc:
            raise Lc3EncoderError(rc, "encode_mixed")

    def encode_frame(self, channel_index, samples_in, buf_out):
        """encode one frame of one channel; len(buf_out) selects the bitrate (lc3_encoder.rs:65,175-191)"""
        samples_in = np.ascontiguousarray(samples_in, dtype=np.int16)
        if not (isinstance(buf_out, np.ndarray) and buf_out.dtype == np.uint8 and buf_out.flags.c_contiguous):
            raise TypeError("buf_out must be a contiguous uint8 numpy array")
        rc = self._L.lc3gpu_encode_frame(self._h, int(channel_index), _ptr(samples_in), int(samples_in.size),
                                         _ptr(buf_out), int(buf_out.size))
        if rc:
            raise Lc3EncoderError(rc, "encode_frame")

    def encode_frame_debug(self, samples_in, nbytes):
        samples_in = np.ascontiguousarray(samples_in, dtype=np.int16)
        out = np.zeros(nbytes, np.uint8)
        dbg = np.zeros(ENC_DBG_FLOATS, np.float32)
        rc = self._L.lc3gpu_encode_frame_debug(self._h, _ptr(samples_in), int(samples_in.size), _ptr(out), nbytes,
                                               _ptr(dbg))
        if rc:
            raise Lc3EncoderError(rc, "encode_frame_debug")
        return out, dbg

    def encode(self, d_pcm, d_out, nbytes, n_frames, stream=None, first_channel=None, n_channels=None, layout="planar"):
        """batch: DEVICE int16[S][T][nf] -> DEVICE uint8[S][T][nbytes] (layout "interleaved": int16[T][nf][S] ->
        uint8[T][S][nbytes]), asynchronous on `stream`"""
        if first_channel is None:
            rc = self._L.lc3gpu_encode_layout(self._h, _layout(layout), _ptr(d_pcm), _ptr(d_out), int(nbytes), int(n_frames),
                                              _ptr(stream))
        else:
            rc = self._L.lc3gpu_encode_range(self._h, int(first_channel), int(n_channels), _ptr(d_pcm), _ptr(d_out),
                                             int(nbytes), int(n_frames), _ptr(stream))
        if rc:
            raise Lc3EncoderError(rc, "encode")

    def encode_vbr(self, d_pcm, d_out, d_nbytes, slot_bytes, n_frames, stream=None):
        """batch with a frame size per frame: DEVICE int16[S][T][nf], DEVICE uint16 d_nbytes[S][T] (each frame's buf_out.len()) ->
        DEVICE uint8[S][T][slot_bytes], frame (s, t) in the first d_nbytes[s][t] bytes of its slot; sizes outside [20, slot_bytes] are
        clamped and counted (size_clamps).  Asynchronous on `stream`"""
        rc = self._L.lc3gpu_encode_vbr(self._h, _ptr(d_pcm), _ptr(d_out), _ptr(d_nbytes), int(slot_bytes), int(n_frames), _ptr(stream))
        if rc:
            raise Lc3EncoderError(rc, "encode_vbr")

    def size_clamps(self):
        """frame sizes encode_vbr has clamped into [20, slot_bytes] on this handle (sticky; waits for the handle's work in flight)"""
        v = ctypes.c_uint64()
        rc = self._L.lc3gpu_encoder_size_clamps(self._h, ctypes.byref(v))
        if rc:
            raise Lc3EncoderError(rc, "size_clamps")
        return int(v.value)

    def stage_event(self, stage, event):
        """every batch call from now on records `event` (the caller's; None clears) behind the kernels of `stage` (ENC_STAGE_*)"""
        rc = self._L.lc3gpu_encoder_stage_event(self._h, int(stage), _event_handle(event))
        if rc:
            raise Lc3EncoderError(rc, "stage_event")
        self._stage_events = getattr(self, "_stage_events", {})
        self._stage_events[int(stage)] = event  # keeps the event alive while it is set

    def timing(self, enable=True):
        """-> (front ms, vector-quantiser ms, back ms, pack ms, batch calls) since the last call; (re)arms recording (enable = n > 1: every n-th batch call)"""
        out = (ctypes.c_double * 5)()
        rc = self._L.lc3gpu_encoder_timing(self._h, int(enable), out)
        if rc:
            raise Lc3EncoderError(rc, "timing")
        return float(out[0]), float(out[1]), float(out[2]), float(out[3]), int(out[4])

    def encode_list(self, channels, d_pcm, d_out, nbytes, n_frames, stream=None):
        """batch over a list of channels (HOST integers, any order, none twice): DEVICE int16[len(channels)][T][nf] -> DEVICE
        uint8[len(channels)][T][nbytes], item i the frames of channel channels[i]; the other channels are left as they were.  Asynchronous
        on `stream`; the list may be reused when the call returns (lc3gpu_encode_list)"""
        ch = _channel_list(channels)
        rc = self._L.lc3gpu_encode_list(self._h, _ptr(ch), int(ch.size), _ptr(d_pcm), _ptr(d_out), int(nbytes), int(n_frames), _ptr(stream))
        if rc:
            raise Lc3EncoderError(rc, "encode_list")

    def encode_mixed_list(self, channels, d_pcm, d_out, n_frames, stream=None):
        """a mixed handle's batch over a list of its streams (HOST descriptor indices, any order, none twice): ragged DEVICE buffers, compact
        in LIST order, as encode_mixed's with the list in place of the descriptor list; every stream at its descriptor's frame size; the
        streams not listed are left as they were.  One launch per kernel; asynchronous on `stream` (lc3gpu_encode_mixed_list)"""
        ch = _channel_list(channels)
        rc = self._L.lc3gpu_encode_mixed_list(self._h, _ptr(ch), int(ch.size), _ptr(d_pcm), _ptr(d_out), int(n_frames), _ptr(stream))
        if rc:
            raise Lc3EncoderError(rc, "encode_mixed_list")

    def encode_mixed_items(self, items, d_pcm, d_out, stream=None):
        """a mixed handle's batch over a list of items `(channel, n_frames[, nbytes])` (HOST, any order, no channel twice): every listed
        stream gets its own number of frames at its own frame size this call (nbytes 0 or left out: the descriptor's).  Ragged DEVICE
        buffers compact in list order: item i's PCM at element offset sum n_frames_j * nf_j, its bytes at sum n_frames_j * nbytes_j.
        One launch per kernel per 24 (configuration, size, count) buckets; asynchronous on `stream` (lc3gpu_encode_mixed_items)"""
        it = _item_list(items)
        rc = self._L.lc3gpu_encode_mixed_items(self._h, _ptr(it), int(it.shape[0]), _ptr(d_pcm), _ptr(d_out), _ptr(stream))
        if rc:
            raise Lc3EncoderError(rc, "encode_mixed_items")

    def encode_mixed_mc_items(self, items, d_pcm, d_out, stream=None):
        """a mixed handle's batch over multi-channel items `(first_channel, n_channels, n_frames[, nbytes])` (HOST; descriptors
        first_channel .. first_channel + n_channels - 1 are one stream's channels, 1..8 of one configuration): WAV sample order in,
        frame order out.  DEVICE buffers compact in list order, item i's PCM int16[T_i][nf_i][C_i] at element sum T_j * nf_j * C_j, its
        bytes uint8[T_i][C_i][nbytes_i] at byte sum T_j * C_j * nbytes_j.  Every channel advances as under encode_mixed_items; launches
        as there; asynchronous on `stream` (lc3gpu_encode_mixed_mc_items)"""
        it = _mc_item_list(items)
        rc = self._L.lc3gpu_encode_mixed_mc_items(self._h, _ptr(it), int(it.shape[0]), _ptr(d_pcm), _ptr(d_out), _ptr(stream))
        if rc:
            raise Lc3EncoderError(rc, "encode_mixed_mc_items")

    def encode_mixed_views(self, views, d_pcm, d_out, stream=None, pcm_elems=None, out_bytes=None):
        """a mixed handle's batch over views (`_view_list`: tuples or dicts of lc3gpu_view's fields): encode_mixed_items with a placement
        per item -- sample n of frame t at d_pcm[pcm_off + t * pcm_pitch + n * pcm_stride], frame t's bytes at d_out[byte_off + t *
        byte_pitch] -- so frames and PCM in rings or in a wide capture buffer are read and written in place.  pcm_elems / out_bytes: the
        buffers' extents (default: the tensors' sizes); every view is checked against them on the host and a call that would leave them
        is refused with LC3GPU_ELENGTH.  Asynchronous on `stream` (lc3gpu_encode_mixed_views)"""
        v = _view_list(views)
        pe = _numel(d_pcm, "pcm_elems") if pcm_elems is None else int(pcm_elems)
        ob = _numel(d_out, "out_bytes") if out_bytes is None else int(out_bytes)
        rc = self._L.lc3gpu_encode_mixed_views(self._h, _ptr(v), int(v.shape[0]), _ptr(d_pcm), pe, _ptr(d_out), ob, _ptr(stream))
        if rc:
            raise Lc3EncoderError(rc, "encode_mixed_views")

    def reset(self, channels=None):
        """every channel (channels=None) or the named ones back to the freshly constructed state from their next call on; no wait"""
        if channels is None:
            rc = self._L.lc3gpu_encoder_reset(self._h)
        else:
            ch = _channel_list(channels)
            rc = self._L.lc3gpu_encoder_reset_channels(self._h, _ptr(ch), int(ch.size))
        if rc:
            raise Lc3EncoderError(rc, "reset")

    def encode_host(self, pcm, out, nbytes, n_frames):
        """HOST int16[S][T][nf] -> HOST uint8[S][T][nbytes] (numpy arrays or raw addresses, e.g. of PinnedBuffer); synchronous (lc3gpu_encode_host)"""
        rc = self._L.lc3gpu_encode_host(self._h, _ptr(pcm), _ptr(out), int(nbytes), int(n_frames))
        if rc:
            raise Lc3EncoderError(rc, "encode_host")

    def bind_stream(self, stream, bind=True):
        """every later batch call comes on `stream` (which outlives the handle): no per-call event of the handle's own (lc3gpu_encoder_bind_stream)"""
        rc = self._L.lc3gpu_encoder_bind_stream(self._h, _ptr(stream), int(bool(bind)))
        if rc:
            raise Lc3EncoderError(rc, "bind_stream")

    def debug_pair_giveup(self):
        """tests only: the device does what a pair half that gives up does (count + host flag)"""
        rc = self._L.lc3gpu_encoder_debug_pair_giveup(self._h)
        if rc:
            raise Lc3EncoderError(rc, "debug_pair_giveup")

    def pair_pending(self):
        """True if the handle's next batch call would return LC3GPU_EPAIR; looks at the flag and leaves it up (lc3gpu_encoder_pair_pending)"""
        rc = self._L.lc3gpu_encoder_pair_pending(self._h)
        if rc < 0:
            raise Lc3EncoderError(rc, "pair_pending")
        return bool(rc)

    def pair_timeouts(self):
        """producer / consumer pair halves of the packer that ever gave up on their partner (include/lc3gpu.h); 0 unless a wave died"""
        v = ctypes.c_uint64()
        rc = self._L.lc3gpu_encoder_pair_timeouts(self._h, ctypes.byref(v))
        if rc:
            raise Lc3EncoderError(rc, "pair_timeouts")
        return int(v.value)

    def state_save(self, channels=None):
        """the state blobs of every channel, or of the named ones (blob i belongs to channels[i])"""
        if channels is not None:
            ch = _channel_list(channels)
            buf = np.zeros(self._L.lc3gpu_encoder_state_size(self._h) * ch.size, np.uint8)
            rc = self._L.lc3gpu_encoder_state_save_channels(self._h, _ptr(ch), int(ch.size), _ptr(buf), buf.size)
            if rc:
                raise Lc3EncoderError(rc, "state_save")
            return buf
        n = self._L.lc3gpu_encoder_state_size(self._h) * self.num_channels
        buf = np.zeros(n, np.uint8)
        rc = self._L.lc3gpu_encoder_state_save(self._h, _ptr(buf), buf.size)
        if rc:
            raise Lc3EncoderError(rc, "state_save")
        return buf

    def state_load(self, buf, channels=None):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        if channels is not None:
            ch = _channel_list(channels)
            if buf.size != self._L.lc3gpu_encoder_state_size(self._h) * ch.size:
                raise ValueError("state blob size does not match the channel list (state_size * len(channels))")
            rc = self._L.lc3gpu_encoder_state_load_channels(self._h, _ptr(ch), int(ch.size), _ptr(buf), buf.size)
            if rc:
                raise Lc3EncoderError(rc, "state_load")
            return
        if buf.size != self._L.lc3gpu_encoder_state_size(self._h) * self.num_channels:
            raise ValueError("state blob size does not match this handle (state_size * num_channels)")
        rc = self._L.lc3gpu_encoder_state_load(self._h, _ptr(buf), buf.size)
        if rc:
            raise Lc3EncoderError(rc, "state_load")

    @classmethod
    def _borrowed(cls, handle, num_channels, frame_duration, sampling_frequency):
        """a handle somebody else owns (a pipeline's): every method works, close() does not destroy it (frame_duration None: a mixed handle)"""
        self = cls.__new__(cls)
        self._L = load_library()
        self.config = Lc3Config(sampling_frequency, frame_duration) if frame_duration is not None else None
        self.num_channels = int(num_channels)
        self._h = ctypes.c_void_p(handle)
        self._borrowed_handle = True
        return self

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed_handle", False):
                self._L.lc3gpu_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Lc3Decoder:
    @staticmethod
    def calc_working_buffer_lengths(num_channels, frame_duration, sampling_frequency):
        """-> (scaler_len, complex_len), lc3_decoder.rs:236-244"""
        out = (ctypes.c_int64 * 2)()
        rc = load_library().lc3gpu_decoder_working_buffer_lengths(num_channels, int(frame_duration),
                                                                  int(sampling_frequency), out)
        if rc:
            raise Lc3DecoderError(rc)
        return tuple(int(v) for v in out)

    def __init__(self, num_channels, frame_duration, sampling_frequency):
        self._L = load_library()
        self.config = Lc3Config(sampling_frequency, frame_duration)
        self.num_channels = int(num_channels)
        h = ctypes.c_void_p()
        rc = self._L.lc3gpu_decoder_create(ctypes.byref(h), self.num_channels, int(frame_duration),
                                           int(sampling_frequency))
        if rc:
            raise Lc3DecoderError(rc, "Lc3Decoder::new")
        self._h = h

    new = classmethod(lambda cls, *a, **k: cls(*a, **k))

    @classmethod
    def mixed(cls, descs):
        """descs = [(fs_hz, frame_us, nbytes), ...] (lc3gpu_decoder_create_mixed)"""
        self = cls.__new__(cls)
        self._L = load_library()
        self.descs = [(int(d[0]), int(d[1]), int(d[2])) for d in descs]
        self.configs = [Lc3Config(d[0], d[1]) for d in self.descs]
        self.config = None
        self.num_channels = len(self.descs)
        h = ctypes.c_void_p()
        rc = self._L.lc3gpu_decoder_create_mixed(ctypes.byref(h), self.num_channels, _desc_array(self.descs))
        if rc:
            raise Lc3DecoderError(rc, "Lc3Decoder::mixed")
        self._h = h
        return self

    def decode_mixed(self, d_in, d_pcm, n_frames, stream=None, d_bad_frame=None):
        rc = self._L.lc3gpu_decode_mixed(self._h, _ptr(d_in), _ptr(d_bad_frame), _ptr(d_pcm), int(n_frames), _ptr(stream))
        if rc:
            raise Lc3DecoderError(rc, "decode_mixed")

    def decode_frame(self, num_bits_per_audio_sample, channel_index, buf_in, samples_out):
        """lc3_decoder.rs:217-234; corrupt frames are concealed, not reported (":138-141")"""
        buf_in = np.ascontiguousarray(buf_in, dtype=np.uint8)
        if not (isinstance(samples_out, np.ndarray) and samples_out.dtype == np.int16 and samples_out.flags.c_contiguous):
            raise TypeError("samples_out must be a contiguous int16 numpy array")
        rc = self._L.lc3gpu_decode_frame(self._h, int(num_bits_per_audio_sample), int(channel_index), _ptr(buf_in),
                                         int(buf_in.size), _ptr(samples_out), int(samples_out.size))
        if rc:
            raise Lc3DecoderError(rc, "decode_frame")

    def decode(self, d_in, d_pcm, nbytes, n_frames, stream=None, d_bad_frame=None, first_channel=None,
               n_channels=None, layout="planar"):
        """batch: DEVICE uint8[S][T][nbytes] -> DEVICE int16[S][T][nf] (layout "interleaved": uint8[T][S][nbytes] ->
        int16[T][nf][S]), asynchronous on `stream`"""
        if first_channel is None:
            rc = self._L.lc3gpu_decode_layout(self._h, _layout(layout), _ptr(d_in), _ptr(d_bad_frame), _ptr(d_pcm), int(nbytes),
                                              int(n_frames), _ptr(stream))
        else:
            rc = self._L.lc3gpu_decode_range(self._h, int(first_channel), int(n_channels), _ptr(d_in),
                                             _ptr(d_bad_frame), _ptr(d_pcm), int(nbytes), int(n_frames), _ptr(stream))
        if rc:
            raise Lc3DecoderError(rc, "decode")

    def decode_vbr(self, d_in, d_nbytes, d_pcm, slot_bytes, n_frames, stream=None, d_bad_frame=None):
        """batch with a frame size per frame: DEVICE uint8[S][T][slot_bytes] (frame (s, t) = the first d_nbytes[s][t] bytes of its slot),
        DEVICE uint16 d_nbytes[S][T] (each frame's buf_in.len(); 0 or above slot_bytes: concealed) -> DEVICE int16[S][T][nf].
        Asynchronous on `stream`"""
        rc = self._L.lc3gpu_decode_vbr(self._h, _ptr(d_in), _ptr(d_nbytes), _ptr(d_bad_frame), _ptr(d_pcm), int(slot_bytes), int(n_frames),
                                       _ptr(stream))
        if rc:
            raise Lc3DecoderError(rc, "decode_vbr")

    def stage_event(self, stage, event):
        """every batch call from now on records `event` (the caller's; None clears) behind the kernels of `stage` (DEC_STAGE_PARSE)"""
        rc = self._L.lc3gpu_decoder_stage_event(self._h, int(stage), _event_handle(event))
        if rc:
            raise Lc3DecoderError(rc, "stage_event")
        self._stage_events = getattr(self, "_stage_events", {})
        self._stage_events[int(stage)] = event

    def timing(self, enable=True):
        """-> (parse-kernel ms, synthesis-kernel ms, batch calls) since the last call; (re)arms recording (enable = n > 1: every n-th batch call)"""
        out = (ctypes.c_double * 3)()
        rc = self._L.lc3gpu_decoder_timing(self._h, int(enable), out)
        if rc:
            raise Lc3DecoderError(rc, "timing")
        return float(out[0]), float(out[1]), int(out[2])

    def decode_frame_debug(self, buf_in, recon_form=1):
        """one frame of channel 0 with stage dumps -> (pcm int16[nf], dbg float32[DBG_FLOATS]); recon_form 0 lane, 1 late, 2 wave"""
        buf_in = np.ascontiguousarray(buf_in, np.uint8)
        out = np.zeros(self.config.nf, np.int16)
        dbg = np.zeros(DBG_FLOATS, np.float32)
        rc = self._L.lc3gpu_decode_frame_debug(self._h, int(recon_form), _ptr(buf_in), int(buf_in.size), _ptr(out), int(out.size), _ptr(dbg))
        if rc:
            raise Lc3DecoderError(rc, "decode_frame_debug")
        return out, dbg

    def synth_debug(self, data, ltpf_active, pitch_index, nbytes, time_in=False):
        """the synthesis half alone on channel 0: a spectrum (ne floats) or, with time_in, the post-filter's input samples (nf floats)
        -> (pcm int16[nf], dbg float32[DBG_FLOATS])"""
        data = np.ascontiguousarray(data, np.float32)
        out = np.zeros(self.config.nf, np.int16)
        dbg = np.zeros(DBG_FLOATS, np.float32)
        rc = self._L.lc3gpu_decoder_synth_debug(self._h, int(bool(time_in)), _ptr(data), int(data.size), int(ltpf_active), int(pitch_index),
                                                int(nbytes), _ptr(out), int(out.size), _ptr(dbg))
        if rc:
            raise Lc3DecoderError(rc, "synth_debug")
        return out, dbg

    def timing_kernels(self, enable=True):
        """-> (parse ms, reconstruction-kernel ms, TNS-kernel ms, synthesis ms, batch calls) since the last call; (re)arms recording (enable = n > 1: every n-th batch call)"""
        out = (ctypes.c_double * 5)()
        rc = self._L.lc3gpu_decoder_timing_kernels(self._h, int(enable), out)
        if rc:
            raise Lc3DecoderError(rc, "timing")
        return float(out[0]), float(out[1]), float(out[2]), float(out[3]), int(out[4])

    def decode_list(self, channels, d_in, d_pcm, nbytes, n_frames, stream=None, d_bad_frame=None):
        """batch over a list of channels (HOST integers, any order, none twice): DEVICE uint8[len(channels)][T][nbytes] (and optional flags
        uint8[len(channels)][T]) -> DEVICE int16[len(channels)][T][nf], item i the frames of channel channels[i]; the other channels keep
        their state and PLC count.  Asynchronous on `stream` (lc3gpu_decode_list)"""
        ch = _channel_list(channels)
        rc = self._L.lc3gpu_decode_list(self._h, _ptr(ch), int(ch.size), _ptr(d_in), _ptr(d_bad_frame), _ptr(d_pcm), int(nbytes), int(n_frames),
                                        _ptr(stream))
        if rc:
            raise Lc3DecoderError(rc, "decode_list")

    def decode_mixed_list(self, channels, d_in, d_pcm, n_frames, stream=None, d_bad_frame=None):
        """a mixed handle's batch over a list of its streams (HOST descriptor indices, any order, none twice): ragged DEVICE buffers,
        compact in LIST order, as decode_mixed's with the list in place of the descriptor list (flags uint8[len(channels)][T]); the streams
        not listed keep their state and PLC count.  One launch per kernel; asynchronous on `stream` (lc3gpu_decode_mixed_list)"""
        ch = _channel_list(channels)
        rc = self._L.lc3gpu_decode_mixed_list(self._h, _ptr(ch), int(ch.size), _ptr(d_in), _ptr(d_bad_frame), _ptr(d_pcm), int(n_frames),
                                              _ptr(stream))
        if rc:
            raise Lc3DecoderError(rc, "decode_mixed_list")

    def decode_mixed_items(self, items, d_in, d_pcm, stream=None, d_bad_frame=None):
        """a mixed handle's batch over a list of items `(channel, n_frames[, nbytes])`, as Lc3Encoder.encode_mixed_items: d_in like its
        d_out, d_bad_frame one flag per frame in item order; frame sizes 1..400 (lc3gpu_decode_mixed_items)"""
        it = _item_list(items)
        rc = self._L.lc3gpu_decode_mixed_items(self._h, _ptr(it), int(it.shape[0]), _ptr(d_in), _ptr(d_bad_frame), _ptr(d_pcm), _ptr(stream))
        if rc:
            raise Lc3DecoderError(rc, "decode_mixed_items")

    def decode_mixed_mc_items(self, items, d_in, d_pcm, stream=None, d_bad_frame=None):
        """a mixed handle's batch over multi-channel items `(first_channel, n_channels, n_frames[, nbytes])`, as
        Lc3Encoder.encode_mixed_mc_items: d_in like its d_out, d_pcm int16[T][nf][C] per item, d_bad_frame uint8[T][C] per item; frame
        sizes 1..400 (lc3gpu_decode_mixed_mc_items)"""
        it = _mc_item_list(items)
        rc = self._L.lc3gpu_decode_mixed_mc_items(self._h, _ptr(it), int(it.shape[0]), _ptr(d_in), _ptr(d_bad_frame), _ptr(d_pcm), _ptr(stream))
        if rc:
            raise Lc3DecoderError(rc, "decode_mixed_mc_items")

    def decode_mixed_views(self, views, d_in, d_pcm, stream=None, d_bad_frame=None, in_bytes=None, pcm_elems=None, n_flags=None):
        """a mixed handle's batch over views, as Lc3Encoder.encode_mixed_views: frame t's bytes at d_in[byte_off + t * byte_pitch], its flag
        at d_bad_frame[flag_off + t * flag_pitch] (when given), its samples written to d_pcm[pcm_off + t * pcm_pitch + n * pcm_stride] and
        nothing else; frame sizes 1..400 (lc3gpu_decode_mixed_views)"""
        v = _view_list(views)
        ib = _numel(d_in, "in_bytes") if in_bytes is None else int(in_bytes)
        pe = _numel(d_pcm, "pcm_elems") if pcm_elems is None else int(pcm_elems)
        nfl = 0 if d_bad_frame is None else (_numel(d_bad_frame, "n_flags") if n_flags is None else int(n_flags))
        rc = self._L.lc3gpu_decode_mixed_views(self._h, _ptr(v), int(v.shape[0]), _ptr(d_in), ib, _ptr(d_bad_frame), nfl, _ptr(d_pcm), pe,
                                               _ptr(stream))
        if rc:
            raise Lc3DecoderError(rc, "decode_mixed_views")

    def reset(self, channels=None):
        """every channel (channels=None) or the named ones back to the freshly constructed state (PLC count 0) from their next call on; no wait"""
        if channels is None:
            rc = self._L.lc3gpu_decoder_reset(self._h)
        else:
            ch = _channel_list(channels)
            rc = self._L.lc3gpu_decoder_reset_channels(self._h, _ptr(ch), int(ch.size))
        if rc:
            raise Lc3DecoderError(rc, "reset")

    def plc_events(self):
        v = ctypes.c_uint64()
        rc = self._L.lc3gpu_decoder_plc_events(self._h, ctypes.byref(v))
        if rc:
            raise Lc3DecoderError(rc, "plc_events")
        return int(v.value)

    def decode_host(self, data, pcm, nbytes, n_frames, bad_frame=None):
        """HOST uint8[S][T][nbytes] -> HOST int16[S][T][nf]; synchronous (lc3gpu_decode_host)"""
        rc = self._L.lc3gpu_decode_host(self._h, _ptr(data), _ptr(bad_frame), _ptr(pcm), int(nbytes), int(n_frames))
        if rc:
            raise Lc3DecoderError(rc, "decode_host")

    def bind_stream(self, stream, bind=True):
        rc = self._L.lc3gpu_decoder_bind_stream(self._h, _ptr(stream), int(bool(bind)))
        if rc:
            raise Lc3DecoderError(rc, "bind_stream")

    def debug_pair_giveup(self):
        rc = self._L.lc3gpu_decoder_debug_pair_giveup(self._h)
        if rc:
            raise Lc3DecoderError(rc, "debug_pair_giveup")

    def pair_pending(self):
        """True if the handle's next batch call would return LC3GPU_EPAIR; looks at the flag and leaves it up (lc3gpu_decoder_pair_pending)"""
        rc = self._L.lc3gpu_decoder_pair_pending(self._h)
        if rc < 0:
            raise Lc3DecoderError(rc, "pair_pending")
        return bool(rc)

    def pair_timeouts(self):
        """producer / consumer pair halves of the parser that ever gave up on their partner (include/lc3gpu.h); 0 unless a wave died"""
        v = ctypes.c_uint64()
        rc = self._L.lc3gpu_decoder_pair_timeouts(self._h, ctypes.byref(v))
        if rc:
            raise Lc3DecoderError(rc, "pair_timeouts")
        return int(v.value)

    def state_save(self, channels=None):
        """the state blobs of every channel, or of the named ones (blob i belongs to channels[i])"""
        if channels is not None:
            ch = _channel_list(channels)
            buf = np.zeros(self._L.lc3gpu_decoder_state_size(self._h) * ch.size, np.uint8)
            rc = self._L.lc3gpu_decoder_state_save_channels(self._h, _ptr(ch), int(ch.size), _ptr(buf), buf.size)
            if rc:
                raise Lc3DecoderError(rc, "state_save")
            return buf
        n = self._L.lc3gpu_decoder_state_size(self._h) * self.num_channels
        buf = np.zeros(n, np.uint8)
        rc = self._L.lc3gpu_decoder_state_save(self._h, _ptr(buf), buf.size)
        if rc:
            raise Lc3DecoderError(rc, "state_save")
        return buf

    def state_load(self, buf, channels=None):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        if channels is not None:
            ch = _channel_list(channels)
            if buf.size != self._L.lc3gpu_decoder_state_size(self._h) * ch.size:
                raise ValueError("state blob size does not match the channel list (state_size * len(channels))")
            rc = self._L.lc3gpu_decoder_state_load_channels(self._h, _ptr(ch), int(ch.size), _ptr(buf), buf.size)
            if rc:
                raise Lc3DecoderError(rc, "state_load")
            return
        if buf.size != self._L.lc3gpu_decoder_state_size(self._h) * self.num_channels:
            raise ValueError("state blob size does not match this handle (state_size * num_channels)")
        rc = self._L.lc3gpu_decoder_state_load(self._h, _ptr(buf), buf.size)
        if rc:
            raise Lc3DecoderError(rc, "state_load")

    _borrowed = Lc3Encoder.__dict__["_borrowed"]

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed_handle", False):
                self._L.lc3gpu_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Companion:
    """what the handle classes of the companion libraries share: the handle of lc3gpu_<_NAME>_create, the descriptors, close / __del__, and
    "call, or raise with the call's name".  A subclass names its object (_NAME), may give its descriptor array a dtype of its own (_DESC_DTYPE;
    default: lc3gpu_stream_desc), and its __init__ passes _create what its create takes beyond descs and max_views"""
    _NAME = None
    _DESC_DTYPE = None

    @staticmethod
    def _desc(d):
        return int(d[0]), int(d[1]), int(d[2])

    def _create(self, descs, max_views, *more):
        self._L = load_library()
        self.descs = [self._desc(d) for d in descs]
        self.num_channels = len(self.descs)
        self.max_views = int(max_views)
        if self._DESC_DTYPE is None:
            arr = _desc_array(self.descs)
        else:
            table = np.zeros(max(1, self.num_channels), self._DESC_DTYPE)
            for k, d in enumerate(self.descs):
                table[k] = d
            arr = _ptr(table)
        h = ctypes.c_void_p()
        rc = getattr(self._L, "lc3gpu_%s_create" % self._NAME)(ctypes.byref(h), self.num_channels, arr, self.max_views, *more)
        if rc:
            raise Lc3GpuError(rc, type(self).__name__ + "::new")
        self._h = h

    def _call(self, fn, *args):
        """lc3gpu_<fn>(handle, *args), or Lc3GpuError(rc, fn)"""
        rc = getattr(self._L, "lc3gpu_" + fn)(self._h, *args)
        if rc:
            raise Lc3GpuError(rc, fn)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, "lc3gpu_%s_destroy" % self._NAME)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ChannelStates(_Companion):
    """a companion with a state per channel on the device: reset and reset_channels (lc3gpu_<_NAME>_reset, lc3gpu_<_NAME>_reset_channels)"""

    def reset(self):
        """every channel starts fresh in its next call -- a zero history, or last = 0, env = 0, hang = 0; waits for nothing, launches nothing"""
        self._call(self._NAME + "_reset")

    def reset_channels(self, channels):
        """the named channels start fresh in their next call"""
        ch = np.ascontiguousarray(np.asarray(channels, np.int32).reshape(-1))
        self._call(self._NAME + "_reset_channels", _ptr(ch) if ch.size else None, int(ch.size))


def _companion_plan_info(name, fn, types, *args):
    """the values <fn>(*args, &out...) of the companion library `name` writes, one per ctypes type of `types`: the plan's own figures, from
    the companion itself (tests and tools)"""
    load_library()  # (the main library first: it brings the companion in, and the one HIP runtime of the process)
    out = [t() for t in types]
    rc = getattr(ctypes.CDLL(companion_library_path(name)), fn)(*args, *[ctypes.byref(o) for o in out])
    if rc:
        raise Lc3GpuError(rc, name + "_plan_info")
    return tuple(o.value for o in out)


class Lc3Inspector(_Companion):
    """lc3gpu_inspector: the status and the side information of every frame of a tick, for the very views the tick passes to
    Lc3Decoder.decode_mixed_views.  descs = [(fs_hz, frame_us, nbytes), ...] as for Lc3Decoder.mixed; max_views = the most views one call
    may name.  Independent of every codec handle; bound to the device current at creation."""
    _NAME = "inspector"

    def __init__(self, descs, max_views):
        self._create(descs, max_views)

    def inspect_mixed_views(self, views, d_in, d_status=None, d_info=None, d_bad_frame=None, stream=None, in_bytes=None, n_status=None, n_info=None,
                            n_flags=None):
        """one launch over all views: frame t of a view has its bytes at d_in[byte_off + t * byte_pitch], its flag at
        d_bad_frame[flag_off + t * flag_pitch] (when given); its status byte goes to d_status[the same index] (uint8) and its record to
        d_info[the same index] (FRAME_INFO_DTYPE, 128 bytes; as a uint8 tensor: 128 elements per record).  At least one of d_status and
        d_info; the extents default to the buffers' sizes (lc3gpu_inspect_mixed_views)"""
        v = _view_list(views)
        ib = _numel(d_in, "in_bytes") if in_bytes is None else int(in_bytes)
        nfl = 0 if d_bad_frame is None else (_numel(d_bad_frame, "n_flags") if n_flags is None else int(n_flags))
        nst = 0 if d_status is None else (_numel(d_status, "n_status") if n_status is None else int(n_status))
        nin = _records(d_info, n_info, FRAME_INFO_DTYPE.itemsize, "n_info")
        self._call("inspect_mixed_views", _ptr(v), int(v.shape[0]), _ptr(d_in), ib, _ptr(d_bad_frame), nfl, _ptr(d_status), nst, _ptr(d_info), nin,
                   _ptr(stream))


def inspector_plan_info(max_nbytes):
    """-> (frames per workgroup, dynamic LDS bytes, upload ring slots) of an inspector call whose largest frame size is max_nbytes"""
    return _companion_plan_info("inspector", "lc3insp_plan_info", (ctypes.c_int, ctypes.c_size_t, ctypes.c_int), int(max_nbytes))


# frame analysis (lc3gpu_analyze_mixed_views): the row lengths of d_bands and d_spec (LC3GPU_BANDS, LC3GPU_SPEC_LINES)
BANDS, SPEC_LINES = 64, 400


class Lc3Analyzer(_Companion):
    """lc3gpu_analyzer: the reconstructed spectrum, the 64 band energies and the total energy of every frame of a tick, for the very views
    the tick passes to Lc3Decoder.decode_mixed_views and Lc3Inspector.inspect_mixed_views, without decoding to PCM.  descs = [(fs_hz,
    frame_us, nbytes), ...] as for Lc3Decoder.mixed; max_views / max_frames = the most views one call may name and the most frames it may
    hold.  Independent of every codec handle; bound to the device current at creation."""

    _NAME = "analyzer"

    def __init__(self, descs, max_views, max_frames):
        self.max_frames = int(max_frames)
        self._create(descs, max_views, self.max_frames)

    def analyze_mixed_views(self, views, d_in, d_energy=None, d_bands=None, d_spec=None, d_bad_frame=None, stream=None, in_bytes=None,
                            n_energy=None, n_bands=None, n_spec=None, n_flags=None):
        """one launch over all views: frame t of a view has its bytes at d_in[byte_off + t * byte_pitch], its flag at d_bad_frame[i] (when
        given) with i = flag_off + t * flag_pitch; its total energy goes to d_energy[i] (float32; -1 for a frame the decoder would
        conceal), its band energies to d_bands[i * 64 ..] and its spectrum to d_spec[i * 400 ..] (float32 rows; d_spec 16-byte aligned).
        At least one of the three; the extents (floats, rows, rows) default to the buffers' sizes (lc3gpu_analyze_mixed_views)"""
        v = _view_list(views)
        ib = _numel(d_in, "in_bytes") if in_bytes is None else int(in_bytes)
        nfl = 0 if d_bad_frame is None else (_numel(d_bad_frame, "n_flags") if n_flags is None else int(n_flags))
        ne = _records(d_energy, n_energy, 4, "n_energy")  # (float32 rows of 1, 64 and 400)
        nbd = _records(d_bands, n_bands, 4 * BANDS, "n_bands")
        nsp = _records(d_spec, n_spec, 4 * SPEC_LINES, "n_spec")
        self._call("analyze_mixed_views", _ptr(v), int(v.shape[0]), _ptr(d_in), ib, _ptr(d_bad_frame), nfl, _ptr(d_energy), ne, _ptr(d_bands), nbd,
                   _ptr(d_spec), nsp, _ptr(stream))


def analyzer_plan_info(max_nbytes):
    """-> (frames per workgroup, dynamic LDS bytes, upload ring slots, words of a frame's scratch column) of an analyzer call whose largest
    frame size is max_nbytes"""
    return _companion_plan_info("analyzer", "lc3ana_plan_info", (ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int), int(max_nbytes))


# room mixes (lc3gpu_mix_mixed_views): the entries of the two room tables (lc3gpu_mix_in, lc3gpu_mix_out, 8 bytes each) and unity gain
MIX_IN_DTYPE = np.dtype([("bus", "<i4"), ("gain_q14", "<i4")])
MIX_OUT_DTYPE = np.dtype([("bus", "<i4"), ("minus", "<i4")])
MIX_UNITY = 16384


def _mix_table(rows, dtype):
    """a sequence of pairs, or an array of the table's dtype -> contiguous HOST array of it"""
    if isinstance(rows, np.ndarray) and rows.dtype == dtype:
        return np.ascontiguousarray(rows.reshape(-1))
    rows = list(rows)
    out = np.zeros(len(rows), dtype)
    for k, r in enumerate(rows):
        out[k] = (int(r[0]), int(r[1]))
    return out


class Lc3Mixer(_Companion):
    """lc3gpu_mixer: the room mixes of a tick, the PCM read where Lc3Decoder.decode_mixed_views wrote it and written where
    Lc3Encoder.encode_mixed_views reads it, in one launch.  descs = [(fs_hz, frame_us, nbytes), ...] as for Lc3Decoder.mixed (only the
    rate and the duration are used); max_views = the most input plus output views one call may name, and the number of buses.
    Independent of every codec handle, of the inspector and of the analyzer; bound to the device current at creation."""

    _NAME = "mixer"

    def __init__(self, descs, max_views):
        self._create(descs, max_views)

    def mix_mixed_views(self, in_views, ins, d_pcm_in, out_views, outs, d_pcm_out, stream=None, in_elems=None, out_elems=None):
        """one launch over all rooms.  ins[i] = (bus, gain_q14) belongs to in_views[i], outs[o] = (bus, minus) to out_views[o]; output o
        gets, sample by sample, the clamped sum of ((in * gain_q14 + 8192) >> 14) over the inputs of its bus, less that term of input
        `minus` (-1: none).  d_pcm_in / d_pcm_out: int16 device buffers that do not overlap; the extents (elements) default to the
        buffers' sizes (lc3gpu_mix_mixed_views)"""
        vi, vo = _view_list(in_views), _view_list(out_views)
        ti, to = _mix_table(ins, MIX_IN_DTYPE), _mix_table(outs, MIX_OUT_DTYPE)
        if ti.shape[0] != vi.shape[0] or to.shape[0] != vo.shape[0]:
            raise ValueError("one (bus, gain_q14) per input view and one (bus, minus) per output view")
        ie = (0 if d_pcm_in is None else _numel(d_pcm_in, "in_elems")) if in_elems is None else int(in_elems)
        oe = (0 if d_pcm_out is None else _numel(d_pcm_out, "out_elems")) if out_elems is None else int(out_elems)
        self._call("mix_mixed_views", _ptr(vi) if vi.shape[0] else None, _ptr(ti) if ti.shape[0] else None, int(vi.shape[0]), _ptr(d_pcm_in), ie,
                   _ptr(vo) if vo.shape[0] else None, _ptr(to) if to.shape[0] else None, int(vo.shape[0]), _ptr(d_pcm_out), oe, _ptr(stream))


def mixer_plan_info():
    """-> (samples of a bus per workgroup, lanes per workgroup, upload ring slots) of a mixer call"""
    return _companion_plan_info("mixer", "lc3mix_plan_info", (ctypes.c_int,) * 3)


# rate conversion (lc3gpu_resample_mixed_views): lc3gpu_rate_desc, 12 bytes
RATE_DESC_DTYPE = np.dtype([("fs_in_hz", "<i4"), ("fs_out_hz", "<i4"), ("frame_us", "<i4")])


class Lc3Resampler(_ChannelStates):
    """lc3gpu_resampler: the rate conversions of a tick, the PCM read where one view array says and written where a second says, in one
    launch, with a FIR history per channel.  descs = [(fs_in_hz, fs_out_hz, frame_us), ...]; max_views = the most pairs of views one
    call may name.  Independent of every codec handle and of the three other companions; bound to the device current at creation."""

    _NAME, _DESC_DTYPE = "resampler", RATE_DESC_DTYPE

    def __init__(self, descs, max_views):
        self._create(descs, max_views)

    def resample_mixed_views(self, in_views, d_pcm_in, out_views, d_pcm_out, stream=None, in_elems=None, out_elems=None):
        """one launch over all listed channels.  in_views[i] and out_views[i] belong together (same channel, same n_frames; a channel
        once per call); every output sample is the clamped, rounded int32 FIR sum of include/lc3gpu.h over the view's input and the
        channel's history, which advances.  d_pcm_in / d_pcm_out: int16 device buffers that do not overlap; the extents (elements)
        default to the buffers' sizes (lc3gpu_resample_mixed_views)"""
        vi, vo = _view_list(in_views), _view_list(out_views)
        if vi.shape[0] != vo.shape[0]:
            raise ValueError("one output view per input view")
        ie = (0 if d_pcm_in is None else _numel(d_pcm_in, "in_elems")) if in_elems is None else int(in_elems)
        oe = (0 if d_pcm_out is None else _numel(d_pcm_out, "out_elems")) if out_elems is None else int(out_elems)
        n = int(vi.shape[0])
        self._call("resample_mixed_views", _ptr(vi) if n else None, _ptr(d_pcm_in), ie, _ptr(vo) if n else None, _ptr(d_pcm_out), oe, n, _ptr(stream))


def resampler_plan_info():
    """-> (output samples of a view per workgroup, lanes per workgroup, upload ring slots, samples of a history buffer) of a resampler call"""
    return _companion_plan_info("resampler", "lc3rs_plan_info", (ctypes.c_int,) * 4)


# PCM levels (lc3gpu_measure_mixed_views): lc3gpu_meter_desc, 24 bytes, and the record of one frame, lc3gpu_level, 32 bytes
METER_DESC_DTYPE = np.dtype([("fs_hz", "<i4"), ("frame_us", "<i4"), ("attack_q15", "<i4"), ("release_q15", "<i4"), ("threshold", "<u4"),
                             ("hang_frames", "<i4")])
LEVEL_DTYPE = np.dtype([("sum_sq", "<i8"), ("env", "<u4"), ("sum", "<i4"), ("min", "<i2"), ("max", "<i2"), ("n_clipped", "<u2"), ("n_cross", "<u2"),
                        ("hang", "<u2"), ("active", "u1"), ("reserved0", "u1"), ("reserved1", "<u4")])
assert METER_DESC_DTYPE.itemsize == 24 and LEVEL_DTYPE.itemsize == 32


class Lc3Meter(_ChannelStates):
    """lc3gpu_meter: the PCM levels and the speech gate of a tick, the PCM read where one view array says it lies, in one launch, with a
    small state per channel (last sample, envelope, hang-over) carried from call to call.  descs = [(fs_hz, frame_us, attack_q15,
    release_q15, threshold, hang_frames), ...]; max_views = the most views one call may name.  Independent of every other object; bound to
    the device current at creation."""

    _NAME, _DESC_DTYPE = "meter", METER_DESC_DTYPE

    @staticmethod
    def _desc(d):
        return tuple(int(x) for x in d)

    def __init__(self, descs, max_views):
        self._create(descs, max_views)

    def measure_mixed_views(self, views, d_pcm, d_active=None, d_levels=None, stream=None, pcm_elems=None, n_active=None, n_levels=None):
        """one launch over all listed channels (a channel once per call).  Frame t of a view gets, at index flag_off + t * flag_pitch, its
        activity byte in d_active (uint8) and its 32-byte record in d_levels (LEVEL_DTYPE, 16-byte aligned); either may be None, not both.
        d_pcm: an int16 device buffer that overlaps neither output.  The extents default to the buffers' sizes: elements of d_pcm, bytes
        of d_active, and for d_levels its bytes / 32 (lc3gpu_measure_mixed_views)"""
        v = _view_list(views)
        pe = (0 if d_pcm is None else _numel(d_pcm, "pcm_elems")) if pcm_elems is None else int(pcm_elems)
        na = (0 if d_active is None else _numel(d_active, "n_active")) if n_active is None else int(n_active)
        nl = _records(d_levels, n_levels, LEVEL_DTYPE.itemsize, "n_levels")
        n = int(v.shape[0])
        self._call("measure_mixed_views", _ptr(v) if n else None, n, _ptr(d_pcm), pe, _ptr(d_active), na, _ptr(d_levels), nl, _ptr(stream))


def meter_plan_info():
    """-> (waves = views of a workgroup, lanes per workgroup, upload ring slots, bytes of a channel's state on the device) of a meter call"""
    return _companion_plan_info("meter", "lc3mtr_plan_info", (ctypes.c_int,) * 4)


class PinnedBuffer:
    """page-locked host memory from lc3gpu_host_alloc as a numpy array (`.array`): what lc3gpu_encode_host / lc3gpu_decode_host copy at the
    PCIe link's rate"""

    def __init__(self, shape, dtype):
        self._L = load_library()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        rc = self._L.lc3gpu_host_alloc(ctypes.byref(p), max(1, n))
        if rc:
            raise Lc3GpuError(rc, "host_alloc")
        self._p = p
        self.array = np.frombuffer((ctypes.c_uint8 * max(1, n)).from_address(p.value), dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            self._L.lc3gpu_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Lc3Pipeline:
    """lc3gpu_pipeline: the caller loop (examples/encode.rs:97-115, examples/decode.rs:93-112) in the arrangement that measured best --
    groups of the channels, each with an encoder handle and a decoder handle of its own on HIP streams of its own"""

    def __init__(self, num_channels, frame_duration, sampling_frequency, n_groups=0):
        self._L = load_library()
        self.config = Lc3Config(sampling_frequency, frame_duration)
        self.num_channels = int(num_channels)
        h = ctypes.c_void_p()
        rc = self._L.lc3gpu_pipeline_create(ctypes.byref(h), self.num_channels, int(frame_duration), int(sampling_frequency), int(n_groups))
        if rc:
            raise Lc3GpuError(rc, "Lc3Pipeline")
        self._h = h
        self._collect_groups(frame_duration, sampling_frequency)

    @classmethod
    def mixed(cls, descs, n_groups=0, group_first=None):
        """streams of different configurations, descs = [(fs_hz, frame_us, nbytes), ...]; group g takes descs[group_first[g]:group_first[g + 1]]
        (None: equal shares of the list); ragged buffers as for Lc3Encoder.mixed (lc3gpu_pipeline_create_mixed)"""
        self = cls.__new__(cls)
        self._L = load_library()
        self.descs = [(int(d[0]), int(d[1]), int(d[2])) for d in descs]
        self.config = None
        self.num_channels = len(self.descs)
        h = ctypes.c_void_p()
        gf = (ctypes.c_int * len(group_first))(*[int(v) for v in group_first]) if group_first is not None else None
        rc = self._L.lc3gpu_pipeline_create_mixed(ctypes.byref(h), self.num_channels, _desc_array(self.descs),
                                                  int(len(group_first) if group_first is not None else n_groups), gf)
        if rc:
            raise Lc3GpuError(rc, "Lc3Pipeline.mixed")
        self._h = h
        self._collect_groups(None, None)
        return self

    def submit_mixed(self, d_pcm, d_bytes, d_pcm_out, n_frames):
        self._check(self._L.lc3gpu_pipeline_submit_mixed(self._h, _ptr(d_pcm), _ptr(d_bytes), _ptr(d_pcm_out), int(n_frames)), "pipeline_submit_mixed")

    def encode_mixed(self, d_pcm, d_bytes, n_frames):
        self._check(self._L.lc3gpu_pipeline_encode_mixed(self._h, _ptr(d_pcm), _ptr(d_bytes), int(n_frames)), "pipeline_encode_mixed")

    def decode_mixed(self, d_bytes, d_pcm_out, n_frames, d_bad_frame=None):
        self._check(self._L.lc3gpu_pipeline_decode_mixed(self._h, _ptr(d_bytes), _ptr(d_bad_frame), _ptr(d_pcm_out), int(n_frames)), "pipeline_decode_mixed")

    def _collect_groups(self, frame_duration, sampling_frequency):
        h = self._h
        self.groups = []
        for g in range(self._L.lc3gpu_pipeline_groups(h)):
            first, n, e, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_void_p(), ctypes.c_void_p()
            rc = self._L.lc3gpu_pipeline_group(h, g, ctypes.byref(first), ctypes.byref(n), ctypes.byref(e), ctypes.byref(d))
            if rc:
                raise Lc3GpuError(rc, "pipeline_group")
            self.groups.append({"first": first.value, "n": n.value,
                                "enc": Lc3Encoder._borrowed(e.value, n.value, frame_duration, sampling_frequency),
                                "dec": Lc3Decoder._borrowed(d.value, n.value, frame_duration, sampling_frequency)})

    def _check(self, rc, what):
        if rc:
            raise Lc3GpuError(rc, what)

    def submit(self, d_pcm, d_bytes, d_pcm_out, nbytes, n_frames):
        self._check(self._L.lc3gpu_pipeline_submit(self._h, _ptr(d_pcm), _ptr(d_bytes), _ptr(d_pcm_out), int(nbytes), int(n_frames)), "pipeline_submit")

    def encode(self, d_pcm, d_bytes, nbytes, n_frames):
        self._check(self._L.lc3gpu_pipeline_encode(self._h, _ptr(d_pcm), _ptr(d_bytes), int(nbytes), int(n_frames)), "pipeline_encode")

    def decode(self, d_bytes, d_pcm_out, nbytes, n_frames, d_bad_frame=None):
        self._check(self._L.lc3gpu_pipeline_decode(self._h, _ptr(d_bytes), _ptr(d_bad_frame), _ptr(d_pcm_out), int(nbytes), int(n_frames)), "pipeline_decode")

    def wait(self):
        self._check(self._L.lc3gpu_pipeline_wait(self._h), "pipeline_wait")

    def join(self, stream=None):
        self._check(self._L.lc3gpu_pipeline_join(self._h, _ptr(stream)), "pipeline_join")

    def follow(self, stream=None):
        self._check(self._L.lc3gpu_pipeline_follow(self._h, _ptr(stream)), "pipeline_follow")

    def mark(self, event):
        """records `event` (torch.cuda.Event that has been recorded once, or a hipEvent_t) behind the last group's latest work"""
        self._check(self._L.lc3gpu_pipeline_mark(self._h, _event_handle(event)), "pipeline_mark")

    def reset(self):
        self._check(self._L.lc3gpu_pipeline_reset(self._h), "pipeline_reset")

    def close(self):
        if getattr(self, "_h", None):
            for g in self.groups:
                g["enc"].close()
                g["dec"].close()
            self._L.lc3gpu_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prof_read():
    """diagnostic build only: per-slot cycles accumulated since the previous call"""
    out = (ctypes.c_ulonglong * 64)()
    rc = load_library().lc3gpu_prof_read(out)
    if rc:
        raise Lc3GpuError(rc, "prof_read")
    return list(out)


def kernel_info(which):
    out = (ctypes.c_int * 5)()
    rc = load_library().lc3gpu_kernel_info(int(which), out)
    if rc:
        raise Lc3GpuError(rc, "kernel_info")
    return dict(zip(["lds_bytes", "vgprs", "sgprs", "scratch_bytes", "max_threads"], list(out)))
