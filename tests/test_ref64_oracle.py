"""The CPU oracle's float stages against the float64 references of tests/ref64.py, at all 12 configurations.

The oracle is pinned to the reference's known-answer vectors at 48 kHz / 10 ms only (tests/test_oracle_semantics.py); here every
float stage of it is held, at every configuration, to a second derivation written from the stage's formula.  Each bound is checked
for teeth by the mutation tests below: the same comparison against a float64 reference given one plausible table error must fail.
The encoder's decisions are held to float64 models in the same way, under the rule and the margins of ref64_check.MARGIN."""
import dataclasses

import numpy as np
import pytest

import oracle_lib as O
import ref64 as R
import ref64_check as C


def run_oracle(cfg, record, sizes=None, spec_flags=0, oracle_flags=None, ltpf=True, decode=True, check_cfg=None):
    """encode (stage by stage) and decode the material of `cfg` through the oracle, checking every stage against ref64 configured
    as `check_cfg` (default `cfg`).  8 kHz has no reference encoder: it is encoded under LC3O_SPEC_8KHZ_ENCODE."""
    pcm, lt = C.material(cfg)
    flags = spec_flags | (R.SPEC_8KHZ_ENCODE if cfg.fs == 8000 else 0) if oracle_flags is None else oracle_flags
    chk = check_cfg or cfg
    jobs = [(pcm[s], nb) for nb in (sizes or C.frame_sizes(cfg)) for s in range(pcm.shape[0])]
    if ltpf:
        jobs += [(lt[s], C.ltpf_size(cfg)) for s in range(lt.shape[0])]
    for x, nb in jobs:
        data = C.oracle_encode_stream(cfg, x, nb, record, spec_flags=flags, check_cfg=chk)
        if decode:
            C.oracle_decode_stream(chk, data, record)


@pytest.mark.parametrize("nf", [60, 80, 120, 160, 180, 240, 320, 360, 480])
def test_dct_iv_every_size(nf):
    """common/dct_iv.rs: the kissfft-based DCT-IV at every nf of the codec (test_dct_iv_run covers 480 only); normwise bound 16 ulp
    (the mdct row of ref64_check.BOUND: fold-free, so the same rounding budget with room)"""
    rng = np.random.default_rng(nf)
    worst = 0.0
    for scale in (1.0, 3e4):
        for _ in range(8):
            x = (rng.standard_normal(nf) * scale).astype(np.float32)
            y = x.copy()
            O.lib().lc3o_kat_dct4(nf, O.P(y))
            worst = max(worst, C.ratio(y, R.dct4(x.astype(np.float64))))
    # a single line: each radix path alone
    for k in range(0, nf, max(1, nf // 12)):
        x = np.zeros(nf, np.float32)
        x[k] = 1.0
        y = x.copy()
        O.lib().lc3o_kat_dct4(nf, O.P(y))
        worst = max(worst, C.ratio(y, R.dct4(x.astype(np.float64))))
    assert worst <= C.BOUND["mdct"], worst


@pytest.mark.parametrize("fs,us", R.CONFIGS)
def test_oracle_stages_against_float64(fs, us):
    cfg = R.config(fs, us)
    rec = C.Record()
    run_oracle(cfg, rec)
    assert not rec.failures(), (rec.failures(), dict(rec.worst))
    # every stage ran, and the material reached the paths it is there for
    for stage in C.BOUND:
        assert rec.count[stage] > 0 or stage == "recon", stage  # (the oracle dumps every intermediate spectrum)
    p = rec.paths
    assert p["tns"] > 0 and p["tns_dec"] > 0
    for b in C.bandwidths(cfg):
        assert p["bw%d" % b] > 0, ("bandwidth index never reached", b, dict(p))
    for t in range(1, 6):
        assert p["ltpf%d" % t] > 0, ("post-filter transition never reached", t, dict(p))
    assert p["saturated"] > 0
    if fs <= 32000:
        assert p["near_nyquist"] > 0
    if fs >= 32000:
        assert p["attack"] > 0
    assert p["bw_near_tie"] + p["nn_near_tie"] <= max(2, rec.count["mdct"] // 100), dict(p)


# ------------------------------------------------------------------------------------------------------------- spec switches
@pytest.mark.parametrize("fs,us,flag", [(8000, 10000, R.SPEC_8KHZ_ENCODE), (8000, 7500, R.SPEC_8KHZ_ENCODE),
                                        (24000, 10000, R.SPEC_TNS_SSWB_STOP), (48000, 10000, R.SPEC_TNS_SSWB_STOP),
                                        (32000, 10000, R.SPEC_BW_CUTOFF_DB), (48000, 7500, R.SPEC_BW_CUTOFF_DB)])
def test_oracle_spec_switches_against_float64(fs, us, flag):
    """A6 / A5 / A7 corrections: the oracle with the bit set against ref64 with the same bit"""
    cfg = R.config(fs, us, spec_flags=flag)
    rec = C.Record()
    run_oracle(cfg, rec, sizes=(100,), ltpf=False, decode=False, oracle_flags=flag)
    assert not rec.failures(), rec.failures()
    if flag == R.SPEC_TNS_SSWB_STOP:
        assert rec.paths["bw2"] > 0 and rec.paths["tns"] > 0
        # and it has teeth: the reference's stop line (200) no longer matches
        bad = C.Record()
        run_oracle(cfg, bad, sizes=(100,), ltpf=False, decode=False, oracle_flags=flag, check_cfg=R.config(fs, us))
        assert bad.worst["tns"] > C.BOUND["tns"], bad.worst["tns"]


# ------------------------------------------------------------------------------------------------------------- mutations
def _mut_window(cfg):
    w = cfg.window.copy()
    w[int(np.argmax(np.abs(w)))] *= 1.0 + 1e-3
    return dataclasses.replace(cfg, window=w)


def _mut_band_edge(cfg):
    b = cfg.bands.copy()
    # the upper edge of band i - 1 up by one line (where every band is one line wide, 8 kHz 7.5 ms, band i becomes empty)
    i = next((i for i in range(cfg.nb // 2, cfg.nb) if b[i + 1] - b[i] > 1), cfg.nb // 2)
    b[i] += 1
    return dataclasses.replace(cfg, bands=b)


def _mut_tns_stop(cfg):
    def f(t):
        return tuple(tuple(fl[:-1]) + ((fl[-1][0], fl[-1][1] - 1),) for fl in t)

    return dataclasses.replace(cfg, tns_enc=f(cfg.tns_enc), tns_dec=f(cfg.tns_dec))


def _mut_ltpf_tap(cfg):
    d = cfg.ltpf_den.copy()
    d[:, 1] += 1e-3
    return dataclasses.replace(cfg, ltpf_den=d)


def _mut_l_den(cfg):
    return dataclasses.replace(cfg, ltpf_l_den=12)


def _mut_nf_start(cfg):
    return dataclasses.replace(cfg, nf_start=cfg.nf_start + 1)


MUTATIONS = {  # name -> (mutation, the stages whose comparison must fail)
    "window coefficient x (1 + 1e-3)": (_mut_window, ("mdct", "imdct")),
    "band edge moved by one line": (_mut_band_edge, ("eb", "sns", "sns_dec")),
    "TNS stop line moved by one": (_mut_tns_stop, ("tns", "tns_dec")),
    "LTPF tap + 1e-3": (_mut_ltpf_tap, ("ltpf",)),
    "noise-filling start moved by one": (_mut_nf_start, ("gain",)),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
@pytest.mark.parametrize("fs,us", [(16000, 7500), (24000, 10000), (44100, 7500), (8000, 7500)])
def test_mutated_reference_fails(name, fs, us):
    """the comparisons have teeth: a float64 reference with one plausible table error must fail them"""
    mut, stages = MUTATIONS[name]
    cfg = R.config(fs, us)
    rec = C.Record()
    run_oracle(cfg, rec, sizes=C.frame_sizes(cfg)[:2], check_cfg=mut(cfg))
    if cfg.nb == cfg.ne and name.startswith("band edge"):
        stages = ("eb",)  # one line per band: a line that changes band keeps a near-equal scale factor
    for s in stages:
        assert rec.worst[s] > C.BOUND[s], (name, s, rec.worst[s])


def test_mutated_44k1_l_den_fails():
    """44.1 kHz filters with l_den = 11 on the 48 kHz tables; the 48 kHz l_den = 12 must not pass"""
    cfg = R.config(44100, 10000)
    rec = C.Record()
    run_oracle(cfg, rec, sizes=(C.frame_sizes(cfg)[1],), check_cfg=_mut_l_den(cfg))
    assert rec.worst["ltpf"] > C.BOUND["ltpf"], rec.worst["ltpf"]


# ------------------------------------------------------------------------------------------------------------- decisions
def run_oracle_decisions(cfg, check_cfg=None):
    """the encoder's decisions of the oracle over decision_jobs against ref64 configured as `check_cfg` -> Decisions"""
    rec = C.Decisions()
    flags = R.SPEC_8KHZ_ENCODE if cfg.fs == 8000 else 0
    for x, nb in C.decision_jobs(cfg):
        C.oracle_encode_stream(cfg, x, nb, rec, spec_flags=flags, check_cfg=check_cfg)
    return rec


@pytest.mark.parametrize("fs,us", R.CONFIGS)
def test_oracle_decisions_against_float64(fs, us):
    """attack detector, TNS analysis, LTPF analysis, rate loop, residual bits and noise level of the oracle against their float64
    models, under the rule of ref64_check.MARGIN: no disagreement beyond a margin, at most 1 % excused, every path reached"""
    cfg = R.config(fs, us)
    rec = run_oracle_decisions(cfg)
    print(rec.table("oracle %d Hz %d us" % (fs, us)))
    assert not rec.unexcused, rec.unexcused[:8]
    assert not rec.failures(), rec.failures()
    assert not rec.over_cap(cfg), rec.over_cap(cfg)
    missing = [k for k in C.decision_paths(cfg) if not rec.paths[k] > 0]
    assert not missing, (missing, dict(rec.paths))


def _cfg_mut(**kw):
    return lambda cfg: dataclasses.replace(cfg, **kw)


def _mut_t2(cfg):
    return dataclasses.replace(cfg, adj_t=(cfg.adj_t[0], R.ADJ_T2[cfg.fs_ind + 1], cfg.adj_t[2]))


def _mut_tns_sub(cfg):
    return dataclasses.replace(cfg, tns_sub=R.TNS_SUB_10)


def _mut_bw_stop(cfg):
    return dataclasses.replace(cfg, nf_bw_stop=tuple(R.NF_BW_STOP_10))


def _mut_att_edge(cfg):
    return dataclasses.replace(cfg, att_window=(cfg.att_window[0], 1 << 30))


def _mut_ari(cfg):
    return dataclasses.replace(cfg, ari_const=tuple(v + 1 for v in cfg.ari_const))


DECISION_MUTATIONS = {  # name -> (configuration at which the constant matters, mutation, the decisions of which one must fail)
    "7.5 ms mem_mem_nc term dropped": ((16000, 7500), _cfg_mut(ltpf_mmnc=False), ("ltpf_active",)),
    "len12p8 96 -> 128 at 7.5 ms": ((24000, 7500), _cfg_mut(ltpf_len12=128), ("pitch_present", "pitch_index", "ltpf_active")),
    "attack factor 8.5 -> 8": ((48000, 10000), _cfg_mut(att_factor=8.0), ("attack",)),
    "7.5 ms attack window's upper edge removed": ((32000, 7500), _mut_att_edge, ("attack",)),
    "gg_off with fs_ind for fs_ind + 1": ((24000, 10000), _cfg_mut(gg_off_rate=2), ("gain", "gg")),
    "nbits_ari's constant off by one": ((16000, 10000), _mut_ari, ("nbits_spec",)),
    "n > ne/2 -> >=": ((32000, 10000), _cfg_mut(ctx_half_strict=False), ("nbits_trunc", "lastnz_trunc", "lsb_mode")),
    "quantiser offset 0.375 -> 0.5": ((8000, 10000), _cfg_mut(q_offset=0.5), ("quant",)),
    "T2 of one rate": ((24000, 7500), _mut_t2, ("gain",)),
    "nf_start 18 -> 24 at 7.5 ms": ((48000, 7500), _cfg_mut(nf_start=24), ("noise",)),
    "bw_stop of 7.5 ms from the 10 ms table": ((44100, 7500), _mut_bw_stop, ("noise",)),
    "TNS gain threshold 1.5 -> 2": ((16000, 7500), _cfg_mut(tns_gain_thresh=2.0), ("tns",)),
    "7.5 ms TNS sub-blocks from 10 ms": ((32000, 7500), _mut_tns_sub, ("tns",)),
    # beyond the list the checks were asked for: integer thresholds that the material brackets
    "t_nbits gate 560 -> 640": ((32000, 10000), _cfg_mut(ltpf_gate=640), ("ltpf_active",)),
    "rate_flag limit 160 -> 200": ((16000, 7500), _cfg_mut(rate_flag_bits=200), ("nbits_trunc", "lastnz_trunc", "lsb_mode")),
    "7.5 ms TNS weighting limit 360 -> 480": ((24000, 7500), _cfg_mut(tns_weight_bits=480), ("nbits_tns", "tns")),
}


@pytest.mark.parametrize("name", sorted(DECISION_MUTATIONS))
def test_mutated_decision_model_fails(name):
    """the decision checks have teeth: a model with one constant bent must disagree with the oracle beyond every excuse, on the
    same material, at a configuration where that constant matters"""
    (fs, us), mut, decisions = DECISION_MUTATIONS[name]
    cfg = R.config(fs, us)
    rec = run_oracle_decisions(cfg, check_cfg=mut(cfg))
    failed = {u[0] for u in rec.unexcused} | set(rec.failures())
    assert failed & set(decisions), (name, sorted(failed))


def test_mutated_8khz_resampling_factor_fails():
    """the 8 kHz resampling factor 0.5 -> 1.  Every LTPF decision is a ratio of correlations of one signal, so the factor changes
    none of them; what it changes is the 12.8 kHz signal itself, which only the oracle shows (lc3o_kat_ltpf_x12): the model's
    signal against it, normwise as the float stages, with the factor and without"""
    cfg = R.config(8000, 10000)
    for bent, check in ((False, cfg), (True, dataclasses.replace(cfg, ltpf_resamp=1.0))):
        rec = C.Record()
        x, nb = C.decision_jobs(cfg)[0]
        C.oracle_encode_stream(cfg, x, nb, rec, spec_flags=R.SPEC_8KHZ_ENCODE, check_cfg=check, x12=True)
        assert rec.count["x12"] > 0
        assert (rec.worst["x12"] > C.X12_BOUND) == bent, rec.worst["x12"]


# ------------------------------------------------------------------------------------------------------------- round trip
# MDCT -> IMDCT + overlap-add of ref64 alone: the windows' perfect reconstruction (table-independent of either implementation).
# Measured residual max |y - x| / max |x| on full-scale noise: 6.1e-8 (8 kHz 7.5 ms) to 8.6e-8 (24 kHz 7.5 ms), the precision of
# the f32 window tables.
ROUND_TRIP_BOUND = 2e-7


@pytest.mark.parametrize("fs,us", R.CONFIGS)
def test_ref64_mdct_round_trip(fs, us):
    cfg = R.config(fs, us)
    cfg = dataclasses.replace(cfg, ne=cfg.nf)  # every line: the codec's empty lines above ne are not the windows' business
    T = 8
    x = np.random.default_rng(1).uniform(-32768.0, 32767.0, (T, cfg.nf))
    m, i = R.Mdct(cfg), R.Imdct(cfg)
    y = np.concatenate([i.run(m.run(x[t])[:cfg.nf]) for t in range(T)])
    xs = x.reshape(-1)
    d = cfg.nf // 4 if us == 10000 else cfg.nf * 8 // 15  # the codec's delay (test_oracle_semantics.py)
    res = np.abs(y[d:] - xs[:-d])[2 * cfg.nf:]  # after the start-up
    rel = res.max() / np.abs(xs).max()
    assert rel <= ROUND_TRIP_BOUND, rel


# ------------------------------------------------------------------------------------------------------------- post-filter
# chosen filter parameters walking all five transitions, with the longest lag (pitch index 511) right after a change of lag
SYNTH_SCHEDULE = [(0, 0), (0, 0), (1, 60), (1, 60), (1, 300), (1, 511), (1, 511), (0, 0), (1, 420), (1, 100), (0, 0), (0, 0)]


def _ltpf_run(cfg, model):
    rng = np.random.default_rng([cfg.fs, cfg.us])
    d = O.Decoder(cfg.fs, cfg.us)
    nb = C.ltpf_size(cfg)
    worst, prev = 0.0, 0.0
    for active, idx in SYNTH_SCHEDULE:
        x = (rng.standard_normal(cfg.nf) * 3000.0).astype(np.float32)
        y = x.copy()
        O.lib().lc3o_kat_dec_ltpf(d.h, active, 1, idx, 8 * nb, O.P(y))
        worst = max(worst, C.ratio(y, model.run(x, active, idx, 8 * nb), np.hypot(np.linalg.norm(x), prev)))
        prev = float(np.linalg.norm(x))
    return worst


class _LinearLtpf(R.Ltpf):
    """the post-filter over an unbounded linear history, without the reference's ring"""

    def _filter(self, xs, ys, i, cn, cd, p, written):
        return super()._filter(xs, ys, i, cn, cd, p, -10 ** 9)


@pytest.mark.parametrize("fs,us", R.CONFIGS)
def test_oracle_post_filter_long_lags(fs, us):
    """at 10 ms the reference's two-frame ring makes the longest lags read, right after a change of lag, the slots
    the frame's first 2.5 ms have just overwritten.  ref64 follows the reference; a plain linear history fails at 10 ms."""
    cfg = R.config(fs, us)
    assert _ltpf_run(cfg, R.Ltpf(cfg)) <= C.BOUND["ltpf"]
    linear = _ltpf_run(cfg, _LinearLtpf(cfg))
    if us == 10000:
        assert linear > 1000 * C.BOUND["ltpf"], linear
    else:
        assert linear <= C.BOUND["ltpf"], linear
