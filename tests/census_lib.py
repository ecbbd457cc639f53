"""Which corners of the LC3 frame format a set of frames reaches: a count of named cells, taken from the oracle alone (its two parser
stages per frame, and an oracle decoder fed frame by frame for the long-term post-filter's transitions and the PCM's saturation).
cells(fs, us) is the table of cells the composed corpus (composed_corpus.py) has to fill in a configuration; census() counts any set of
streams against the same names.  Test infrastructure only."""
import collections
import math
import re

import numpy as np

import compose_lib as C
import inspect_lib as I
import oracle_lib as O

FLOOR = 4  # frames per cell and configuration below which a cell counts as empty
PITCH_VALUES = (0, 379, 380, 381, 438, 439, 440, 511)  # both ends of the three ranges of the pitch index


def t_nbits(us, nbytes):
    """the bit count the decoder's filter gain is chosen by (oracle/lc3_dec.c, lc3o_dec_ltpf)"""
    return 8 * nbytes if us == 10000 else int(math.floor(8 * nbytes * 10.0 / 7.5 + 0.5))


def gain_class(fs, us, nbytes):
    """0 .. 3: the four gains 0.4 .. 0.25; 4: the zero-gain branch"""
    t, sf = t_nbits(us, nbytes), 80 * C.fs_index(fs)
    return sum(t >= thr + sf for thr in (320, 400, 480, 560))


def gain_edge_sizes(fs, us):
    """[(j, size one byte below threshold j, smallest size at it)]"""
    out = []
    for j in range(4):
        at = next(n for n in range(1, 401) if gain_class(fs, us, n) > j)
        out.append((j, at - 1, at))
    return out


def rate_flag_sizes(fs):
    n = 20 + 20 * C.fs_index(fs)  # nbits > 160 + 160 * fs_ind
    return n, n + 1


def weighting_sizes(us):
    n = 60 if us == 10000 else 45  # nbits < 480 / 360
    return n - 1, n


def pitch_lag(fs, pitch_index):
    """(pitch_int, pitch_frac) of an active filter, as lc3o_dec_ltpf computes them (float64)"""
    pi = pitch_index
    if pi >= 440:
        p_i, p_fr = pi - 283, 0.0
    elif pi >= 380:
        p_i = pi // 2 - 63
        p_fr = float(2 * pi - 4 * p_i - 252)
    else:
        p_i = pi // 4 + 32
        p_fr = float(pi + 128 - 4 * p_i)
    pitch_fs = (p_i + p_fr / 4.0) * (8000.0 * math.ceil(fs / 8000.0) / 12800.0)
    p_up = int(pitch_fs * 4.0 + 0.5)
    return p_up // 4, p_up % 4


def pitch_range(pitch_index):
    return "low" if pitch_index < 380 else ("mid" if pitch_index < 440 else "high")


def escape_depth(a, b):
    m = max(abs(int(a)), abs(int(b)))
    return max(0, m.bit_length() - 2)


def frame_tags(fs, us, frame, ins=None):
    """(tags of one frame, its record, its spectrum or None)"""
    ins = ins or I.OracleInspector(fs, us)
    frame = np.asarray(frame, np.uint8)
    rec = ins.record(frame)
    tags = ["status=%d" % rec[0]]
    if rec[0]:
        return tags, rec, None
    cfg, n = ins.c, len(frame)
    ne = cfg.ne
    w = rec[2:22]
    x = np.array(ins.x[:ne], np.int64)
    bw, lastnz, lsb_mode, gg = int(w[0]), int(w[1]), int(w[2]), int(w[3])
    _, rate_flag, weighting = C.derived(fs, us, n)
    tags += ["bw=%d" % bw, "lsb_mode=%d" % lsb_mode, "rate_flag=%d" % (rate_flag != 0), "gg=%s" % (gg if gg in (0, 255) else "other")]
    present, active, pidx = int(w[16]), int(w[17]), int(w[18])
    if not present:
        tags.append("pitch=absent")
    else:
        how = "active" if active else "inactive"
        tags.append("pitch=%s/%s" % (pitch_range(pidx), how))
        if pidx in PITCH_VALUES:
            tags.append("pitch_index=%d/%s" % (pidx, how))
        if active:
            tags.append("ltpf_gain=%d" % gain_class(fs, us, n))
            for j, below, at in gain_edge_sizes(fs, us):
                if n in (below, at):
                    tags.append("ltpf_edge=%d/%s" % (j, "below" if n == below else "at"))
    orders = [int(ins.ad.rc_order[0]), int(ins.ad.rc_order[1])]
    for f in range(int(w[4])):
        tags.append("tns%d=%d" % (f, orders[f]))
        if orders[f]:
            tags.append("tns%d=%d/w=%d" % (f, orders[f], weighting))
            for k in range(orders[f]):
                tags.append("rc[%d]=%d" % (8 * f + k, ins.ad.rc_i[8 * f + k]))
    if any(orders[:int(w[4])]) and lastnz <= (12 if us == 10000 else 9):
        tags.append("tns_past_lastnz")
    tags.append("lastnz=%s" % {2: "2", ne // 2: "ne/2", ne // 2 + 2: "ne/2+2", ne: "ne"}.get(lastnz, "other"))
    tags.append("escape=%d" % max(escape_depth(x[k], x[k + 1]) for k in range(0, lastnz, 2)))
    nnz = int((x != 0).sum())
    tags.append("noise=%d/%s" % (w[19], "zero" if nnz == 0 else ("sparse" if 4 * nnz <= ne else "dense")))
    if ins.ad.is_zero_frame:
        tags.append("zero_frame_flag")
    shape = 2 * int(w[14]) + int(w[13])
    top, (b_max, _) = C.sns_index_limits()
    idx_a, idx_b = int(w[11]) & 0xFFFFFFFF, int(w[12]) & 0xFFFFFFFF
    tags += ["ind_lf=%d" % w[7], "ind_hf=%d" % w[8], "sns=%d/g=%d" % (shape, w[15])]
    if idx_a in (0, top[shape]):
        tags.append("sns=%d/idx_a=%s" % (shape, "max" if idx_a else "0"))
    if shape == 0 and idx_b in (0, b_max):
        tags.append("sns=0/idx_b=%s" % ("max" if idx_b else "0"))
    if lsb_mode == 0 and nnz:
        tags.append("res=%s" % ("all" if ins.ad.n_residual_bits == nnz else "budget"))
    if lsb_mode:
        # the lsb walk refines pair by pair; where every coded magnitude is odd (the composed frames), a refined value is odd and an
        # unrefined one even, so a budget that ended between the two values of a pair leaves an odd value beside an even one
        deep = [k for k in range(0, lastnz, 2) if escape_depth(x[k], x[k + 1]) > 0]
        if any(x[k] & 1 and not x[k + 1] & 1 for k in deep):
            tags.append("lsb_cut_mid_pair")
    return tags, rec, x


def census(fs, us, streams):
    """streams: sequences of frames (uint8 arrays, each of its own size) -> Counter of cell names over all frames"""
    out = collections.Counter()
    ins = I.OracleInspector(fs, us)
    for frames in streams:
        dec = O.Decoder(fs, us)
        prev_active, prev_lag = False, (0, 0)
        for fr in frames:
            tags, rec, _ = frame_tags(fs, us, fr, ins)
            _, pcm = dec.decode_frame(fr)
            active = rec[0] == 0 and bool(rec[19])
            lag = pitch_lag(fs, int(rec[20])) if active else (0, 0)
            trans = 1 if not active and not prev_active else 2 if active and not prev_active else 3 if not active else 4 if lag == prev_lag else 5
            tags.append("ltpf_trans=%d" % trans if trans in (1, 3) else "ltpf_trans=%d/frac=%d" % (trans, lag[1]))
            prev_active, prev_lag = active, lag
            hi, lo = bool((pcm == 32767).any()), bool((pcm == -32768).any())
            if hi and lo:
                tags.append("pcm=saturates_both_ways")
            out.update(tags)
    return out


def cells(fs, us):
    """the cells of the composed corpus that exist in a configuration: each must hold at least FLOOR frames"""
    fi, ne = C.fs_index(fs), I.config(fs, us).ne
    nfilt = 2 if fi >= 3 else 1
    top, _ = C.sns_index_limits()
    out = ["pitch_index=%d/active" % v for v in PITCH_VALUES]
    out += ["pitch=%s/inactive" % r for r in ("low", "mid", "high")] + ["pitch=absent"]
    fracs = sorted({pitch_lag(fs, p)[1] for p in range(512)})
    out += ["ltpf_trans=%d/frac=%d" % (t, f) for t in (2, 4, 5) for f in fracs] + ["ltpf_trans=3"]
    out += ["ltpf_gain=%d" % k for k in range(5)]
    out += ["ltpf_edge=%d/%s" % (j, s) for j in range(4) for s in ("below", "at")]
    out += ["bw=%d" % b for b in range(fi + 1)]
    if C.NBITS_BW[fi] and fi + 1 < (1 << C.NBITS_BW[fi]):
        out.append("status=%d" % (I.SIDE_INFO + 2))  # bandwidth index max + 1 (where the field can hold it)
    out += ["tns%d=%d/w=%d" % (f, k, w) for f in range(nfilt) for k in range(1, 9) for w in (0, 1)]
    out += ["rc[%d]=%d" % (p, v) for p in range(8 * nfilt) for v in (0, 16)]
    out += ["tns_past_lastnz", "lastnz=2", "lastnz=ne/2", "lastnz=ne/2+2", "lastnz=ne", "rate_flag=0", "rate_flag=1"]
    out += ["escape=%d" % d for d in range(14)]
    out += ["lsb_mode=0", "lsb_mode=1", "lsb_cut_mid_pair", "res=all", "res=budget"]
    out += ["noise=%d/%s" % (k, s) for k in range(8) for s in ("zero", "sparse")] + ["zero_frame_flag"]
    out += ["ind_lf=%d" % k for k in range(32)] + ["ind_hf=%d" % k for k in range(32)]
    out += ["sns=%d/g=%d" % (s, g) for s in range(4) for g in (0, C.SNS_GAINS[s] - 1)]
    out += ["sns=%d/idx_a=%s" % (s, v) for s in range(4) for v in ("0", "max")] + ["sns=0/idx_b=0", "sns=0/idx_b=max"]
    out += ["status=%d" % (I.SIDE_INFO + 4), "status=%d" % (I.SIDE_INFO + 5)]  # the first invalid joint index of either width
    out += ["gg=0", "gg=255", "pcm=saturates_both_ways"]
    return out


def report(counts):
    """the census as lines of text, cells grouped by their name before '='"""
    natural = lambda name: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]
    groups = collections.OrderedDict()
    for k in sorted(counts, key=natural):
        groups.setdefault(k.split("=")[0], []).append("%s:%d" % (k.split("=", 1)[1] if "=" in k else "", counts[k]))
    return "\n".join("%-24s %s" % (g, "  ".join(v)) for g, v in groups.items())
