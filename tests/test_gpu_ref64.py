"""The HIP kernels' float stages against the float64 references of tests/ref64.py, at all 12 configurations (run with -m gpu).

The same material and bounds as tests/test_ref64_oracle.py, on the device's own stage dumps: lc3gpu_encode_frame_debug (MDCT,
band energies, SNS, TNS, decisions), lc3gpu_decode_frame_debug in all three reconstruction forms, lc3gpu_decoder_synth_debug (IMDCT
and post-filter with chosen filter parameters), and one batch decode through the production kernels against a float64 decode.
The encoder's decisions (attack, TNS and LTPF analysis, rate loop, residual bits, noise level) are held to their float64 models
under the margins measured on the oracle (ref64_check.MARGIN), by default and with the sequential sums forced."""
import importlib

import numpy as np
import pytest

import oracle_lib as O
import ref64 as R
import ref64_check as C
from test_gpu_parity import gpu_decode

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("lc3-codec_amd")
synth = importlib.import_module("lc3-codec_amd.synth")


def _jobs(cfg, sizes=None, ltpf=True):
    pcm, lt = C.material(cfg)
    jobs = [(pcm[s], nb) for nb in (sizes or C.frame_sizes(cfg)) for s in range(pcm.shape[0])]
    if ltpf:
        jobs += [(lt[s], C.ltpf_size(cfg)) for s in range(lt.shape[0])]
    return jobs


def _enc_flags(cfg):
    return cfg.spec_flags | (R.SPEC_8KHZ_ENCODE if cfg.fs == 8000 else 0)


def device_encoder_check(cfg, rec, sizes=None, ltpf=True):
    parser = C.Parser(cfg.fs, cfg.us)
    for x, nb in _jobs(cfg, sizes, ltpf):
        enc = pkg.Lc3Encoder(1, cfg.us, cfg.fs, spec_flags=_enc_flags(cfg))
        chk = C.EncoderCheck(cfg, rec, parser)
        for t in range(x.shape[0]):
            out, dbg = enc.encode_frame_debug(x[t], nb)
            chk.frame(x[t], dbg, out)


@pytest.mark.parametrize("fs,us", R.CONFIGS)
def test_device_encoder_stages_against_float64(fs, us):
    cfg = R.config(fs, us)
    rec = C.Record()
    device_encoder_check(cfg, rec)
    assert not rec.failures(), (rec.failures(), dict(rec.worst))
    print("encoder", fs, us, {k: round(v, 2) for k, v in sorted(rec.worst.items())})
    for stage in ("mdct", "eb", "sns", "tns"):
        assert rec.count[stage] > 0, stage
    for b in C.bandwidths(cfg):
        assert rec.paths["bw%d" % b] > 0, b
    if fs >= 32000:
        assert rec.paths["attack"] > 0
    if fs <= 32000:
        assert rec.paths["near_nyquist"] > 0


def device_decisions(fs, us):
    """the encoder's decisions of the device over decision_jobs (one stream per handle) under the oracle's margins: the checker,
    the path assertions and the cap of tests/test_ref64_oracle.py::test_oracle_decisions_against_float64"""
    cfg = R.config(fs, us)
    rec = C.Decisions()
    parser = C.Parser(fs, us)
    for x, nb in C.decision_jobs(cfg):
        enc = pkg.Lc3Encoder(1, us, fs, spec_flags=_enc_flags(cfg))
        chk = C.EncoderCheck(cfg, rec, parser)
        for t in range(x.shape[0]):
            out, dbg = enc.encode_frame_debug(x[t], nb)
            chk.frame(x[t], dbg, out)
    print(rec.table("device %d Hz %d us" % (fs, us)))
    assert not rec.unexcused, rec.unexcused[:8]
    assert not rec.failures(), rec.failures()
    assert not rec.over_cap(cfg), rec.over_cap(cfg)
    missing = [k for k in C.decision_paths(cfg) if not rec.paths[k] > 0]
    assert not missing, (missing, dict(rec.paths))


@pytest.mark.parametrize("fs,us", R.CONFIGS)
def test_device_decisions_against_float64(fs, us):
    device_decisions(fs, us)


def test_device_decisions_with_sequential_sums():
    """the gain bisection and the noise level are the decisions that the kernels take from a tree sum when it is safely off the
    threshold (tests/test_gpu_parity.py::test_sequential_sum_path_of_guarded_decisions); with LC3GPU_SEQ_SUMS=1, read when a handle
    is created, every one of them takes the sequential sum instead: the same check in a fresh process with it set"""
    import os
    import subprocess
    import sys

    code = (
        "import sys; sys.path.insert(0, 'tests')\n"
        "import test_gpu_ref64 as t\n"
        "t.device_decisions(48000, 10000)\n"
        "t.device_decisions(16000, 7500)\n"
        "print('seq decisions ok')\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LC3GPU_SEQ_SUMS="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "seq decisions ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("fs,us,flag", [(8000, 10000, R.SPEC_8KHZ_ENCODE), (24000, 10000, R.SPEC_TNS_SSWB_STOP),
                                        (48000, 10000, R.SPEC_TNS_SSWB_STOP), (32000, 10000, R.SPEC_BW_CUTOFF_DB),
                                        (48000, 7500, R.SPEC_BW_CUTOFF_DB)])
def test_device_spec_switches_against_float64(fs, us, flag):
    cfg = R.config(fs, us, spec_flags=flag)
    rec = C.Record()
    device_encoder_check(cfg, rec, sizes=(100,), ltpf=False)
    assert not rec.failures(), rec.failures()
    if flag == R.SPEC_TNS_SSWB_STOP:
        assert rec.paths["bw2"] > 0 and rec.paths["tns"] > 0


@pytest.mark.parametrize("form", [0, 1, 2])  # lane (full batches), late (single frames), wave (wave-per-frame kernels)
@pytest.mark.parametrize("fs,us", R.CONFIGS)
def test_device_decoder_stages_against_float64(fs, us, form):
    cfg = R.config(fs, us)
    rec = C.Record()
    parser = C.Parser(fs, us)
    for x, nb in _jobs(cfg, sizes=(20, 400)):
        data = O.encode_batch(x[None], nb, fs, us, spec_flags=_enc_flags(cfg))[0]
        dec = pkg.Lc3Decoder(1, us, fs)
        chk = C.DecoderCheck(cfg, rec, parser)
        for t in range(data.shape[0]):
            pcm, dbg = dec.decode_frame_debug(data[t], recon_form=form)
            chk.frame(data[t], dbg, pcm)
    assert not rec.failures(), (rec.failures(), dict(rec.worst))
    print("decoder form", form, fs, us, {k: round(v, 2) for k, v in sorted(rec.worst.items())})
    need = ("gain", "tns_dec", "sns_dec", "imdct", "ltpf") if form != 2 else ("recon", "imdct", "ltpf")
    for stage in need:  # the late form (1) supplies every stage
        assert rec.count[stage] > 0, (form, stage)
    for t in range(1, 6):
        assert rec.paths["ltpf%d" % t] > 0, ("post-filter transition never reached", t)
    assert rec.paths["tns_dec"] > 0 and rec.paths["saturated"] > 0


# pitch indices: short and long lags (the longest, index 511, reaches beyond one 10 ms frame at 48 kHz: SURVEY A10's ring)
SYNTH_SCHEDULE = [(0, 0), (0, 0), (1, 60), (1, 60), (1, 300), (1, 511), (1, 511), (0, 0), (1, 420), (1, 100), (0, 0), (0, 0)]


@pytest.mark.parametrize("fs,us", R.CONFIGS)
def test_device_synthesis_against_float64(fs, us):
    """lc3gpu_decoder_synth_debug with chosen post-filter parameters walking all five transitions, at a frame size with a non-zero
    filter gain and at one above the A11 limit (gain 0)"""
    cfg = R.config(fs, us)
    rng = np.random.default_rng([fs, us])
    for nb in (C.ltpf_size(cfg), 100):
        rec = C.Record()
        dec = pkg.Lc3Decoder(1, us, fs)
        imdct, ltpf = R.Imdct(cfg), R.Ltpf(cfg)
        prev = (0.0, 0.0)
        for active, idx in SYNTH_SCHEDULE:
            spec = (rng.standard_normal(cfg.ne) * 3000.0 / np.sqrt(1.0 + np.arange(cfg.ne) / 8.0)).astype(np.float32)
            pcm, dbg = dec.synth_debug(spec, active, idx, nb)
            x = dbg[C.D_IMDCT:C.D_IMDCT + cfg.nf].astype(np.float64)
            rec.add("imdct", C.ratio(x, imdct.run(spec), np.hypot(np.linalg.norm(spec), prev[0])))
            y = dbg[C.D_LTPF:C.D_LTPF + cfg.nf]
            rec.add("ltpf", C.ratio(y, ltpf.run(x, active, idx, 8 * nb), np.hypot(np.linalg.norm(x), prev[1])))
            rec.paths["ltpf%d" % ltpf.trans] += 1
            prev = (float(np.linalg.norm(spec)), float(np.linalg.norm(x)))
            assert np.all(np.abs(pcm.astype(np.int64) - R.output_pcm(y)) <= 1)
        assert not rec.failures(), (nb, rec.failures())
        assert all(rec.paths["ltpf%d" % t] > 0 for t in range(1, 6)), dict(rec.paths)


# ------------------------------------------------------------------------------------------------------------------ batch
# share of samples at +-1 from the float64 decode over this material: 4.9e-4 (16 kHz 10 ms) to 1.23e-3 (48 kHz 7.5 ms) at the 12
# configurations, the oracle's decode and the device's alike (they are bit-identical).  The bound is four times the largest; a
# stage error costs far more (the mutation checks of tests/test_ref64_oracle.py).
BATCH_PM1_SHARE = 5e-3


@pytest.mark.parametrize("fs,us", R.CONFIGS)
def test_batch_decode_against_float64_decode(fs, us):
    """the production kernels (gpu_decode, default forms) on a batch, against a decode whose only non-float64 part is the oracle's
    integer parser: max |diff| <= 1 LSB and few +-1 samples"""
    cfg = R.config(fs, us)
    S, T = 6, 150
    pcm = np.concatenate([synth.make_pcm(4, T, cfg.nf, fs, seed=21), synth.make_ltpf_pcm(cfg.nf, fs, n_frames=T)[:2]])
    nb = C.ltpf_size(cfg) + 10
    data = O.encode_batch(pcm, nb, fs, us, spec_flags=_enc_flags(cfg))
    got = gpu_decode(data, cfg.nf, fs, us).astype(np.int64)
    parser = C.Parser(fs, us)
    n = n1 = 0
    for s in range(S):
        want, concealed = C.float64_decode_stream(cfg, data[s], parser)
        if concealed:
            continue
        d = np.abs(got[s] - want)
        assert d.max() <= 1, (s, int(d.max()))
        n += d.size
        n1 += int(np.sum(d == 1))
    assert n >= 4 * T * cfg.nf
    share = n1 / n
    print("batch", fs, us, "+-1 share %.2e" % share)
    assert share <= BATCH_PM1_SHARE, share
