"""float64 references of the codec's float stages, written from their definitions (numpy only).

A second derivation, independent of the oracle (oracle/*.c) and of the device code (lc3-codec_amd/csrc/*.h): every stage below is
the formula of the stage, evaluated in float64 over whole vectors, not a transliteration of either restatement.  Each one cites the
reference (ninjasource/lc3-codec v0.2.0, src/) at the lines that define it, and follows the reference's deviations from the LC3
specification that touch it.  The only constants taken from the repository are the
tables of tables/lc3_tables.h, parsed here (the f32 bit patterns become float32 values, then float64).

Integer stages are not restated: side information, the arithmetic decoder, MPVQ de-enumeration, the SNS vector search, the rate loop
and the packer.  Their integer outputs are inputs here.

`Cfg` holds every table a stage reads, so that a test can hand a stage a deliberately wrong table (tests/test_ref64_oracle.py's
mutation checks) with dataclasses.replace."""
import dataclasses
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES_H = os.path.join(ROOT, "tables", "lc3_tables.h")

# LC3O_SPEC_* / LC3GPU_SPEC_*: opt-in corrections of the reference's deviations that change a float stage here
SPEC_8KHZ_ENCODE = 1  # A6
SPEC_TNS_SSWB_STOP = 2  # A5
SPEC_BW_CUTOFF_DB = 4  # A7

_tables = None


def tables():
    """name -> numpy array of every table in tables/lc3_tables.h (`_BITS` arrays as float64 of their f32 values)"""
    global _tables
    if _tables is None:
        with open(TABLES_H) as f:
            text = f.read()
        out = {}
        pat = re.compile(r"LC3_TABLE_QUAL\s+(u?int\d+_t)\s+LC3T_(\w+?)((?:\[\d+\])+)\s+LC3_TABLE_ALIGN\s*=\s*\{(.*?)\};", re.S)
        for ty, name, dims, body in pat.findall(text):
            shape = tuple(int(d) for d in re.findall(r"\[(\d+)\]", dims))
            vals = [int(v.rstrip("uU"), 0) for v in re.findall(r"-?0x[0-9a-fA-F]+u?|-?\d+", body)]
            a = np.array(vals, np.int64).reshape(shape)
            if name.endswith("_BITS") and ty == "uint32_t":
                a = a.astype(np.uint32).view(np.float32).astype(np.float64)
                name = name[:-5]
            out[name] = a
        _tables = out
    return _tables


# --------------------------------------------------------------------------------------------------------------------------- config
# encoder/temporal_noise_shaping.rs:119-196: per bandwidth index, (start, stop) of each filter and the three autocorrelation
# sub-blocks.  10 ms p_bw = 2 stops at 200 although its sub-blocks run to 240.
TNS_ENC_10 = [[(12, 80)], [(12, 160)], [(12, 200)], [(12, 160), (160, 320)], [(12, 200), (200, 400)]]
TNS_ENC_75 = [[(9, 60)], [(9, 120)], [(9, 180)], [(9, 120), (120, 240)], [(9, 150), (150, 300)]]
# decoder/temporal_noise_shaping.rs:90-113: the decoder's filter ranges (12..240 at 10 ms p_bw 2: the specification's)
TNS_DEC_10 = [[(12, 80)], [(12, 160)], [(12, 240)], [(12, 160), (160, 320)], [(12, 200), (200, 400)]]
TNS_DEC_75 = [[(9, 60)], [(9, 120)], [(9, 180)], [(9, 120), (120, 240)], [(9, 150), (150, 300)]]
# decoder/noise_filling.rs:20-35: the last line of each bandwidth index
NF_BW_STOP_10 = [80, 160, 240, 320, 400]
NF_BW_STOP_75 = [60, 120, 180, 240, 300]


@dataclasses.dataclass(frozen=True)
class Cfg:
    fs: int
    us: int
    fs_ind: int
    nf: int
    ne: int
    nb: int
    z: int
    window: np.ndarray  # 2 nf taps, tables/mdct_windows.rs
    bands: np.ndarray  # nb + 1 band edges, tables/band_index_tables.rs
    tns_enc: tuple  # per bandwidth index: ((start, stop), ...)
    tns_dec: tuple
    nf_start: int
    nf_width: int
    nf_bw_stop: tuple
    ltpf_l_den: int
    ltpf_num: np.ndarray  # [4][taps] per gain index
    ltpf_den: np.ndarray  # [4][taps] per pitch fraction
    spec_flags: int = 0

    @property
    def ten_ms(self):
        return self.us == 10000

    def __hash__(self):
        return hash((self.fs, self.us, self.spec_flags))


def config(fs, us, spec_flags=0):
    """common/config.rs:42-100 and the per-rate tables of each stage"""
    T = tables()
    fs_ind = {8000: 0, 16000: 1, 24000: 2, 32000: 3, 44100: 4, 48000: 4}[fs]
    ten = us == 10000
    nf = (80, 160, 240, 320, 480)[fs_ind] if ten else (60, 120, 180, 240, 360)[fs_ind]
    ne = 400 if nf == 480 else (300 if nf == 360 else nf)
    nb = 60 if (fs == 8000 and not ten) else 64
    z = 3 * nf // 8 if ten else 7 * nf // 30
    wname = ("W_N%d_10MS" if ten else "W_N%d_7P5MS") % nf
    rate = (8000, 16000, 24000, 32000, 48000)[fs_ind]  # 44.1 kHz runs on the 48 kHz layout (config.rs:53-60)
    bname = ("I_%d_10MS" if ten else "I_%d_7P5MS") % rate
    tns_enc = [list(f) for f in (TNS_ENC_10 if ten else TNS_ENC_75)]
    if ten and spec_flags & SPEC_TNS_SSWB_STOP:
        tns_enc[2] = [(12, 240)]  # A5 corrected
    # decoder/long_term_post_filter.rs:104-115: l_den per rate, 44.1 kHz 11 on the 48 kHz tables
    l_den = {8000: 4, 16000: 4, 24000: 6, 32000: 8, 44100: 11, 48000: 12}[fs]
    trate = 48000 if fs == 44100 else fs
    return Cfg(fs=fs, us=us, fs_ind=fs_ind, nf=nf, ne=ne, nb=nb, z=z, window=T[wname].copy(), bands=T[bname].copy(),
               tns_enc=tuple(tuple(f) for f in tns_enc), tns_dec=tuple(tuple(f) for f in (TNS_DEC_10 if ten else TNS_DEC_75)),
               nf_start=24 if ten else 18, nf_width=3 if ten else 2, nf_bw_stop=tuple(NF_BW_STOP_10 if ten else NF_BW_STOP_75),
               ltpf_l_den=l_den, ltpf_num=T["TAB_LTPF_NUM_%d" % trate].copy(), ltpf_den=T["TAB_LTPF_DEN_%d" % trate].copy(),
               spec_flags=spec_flags)


CONFIGS = [(fs, us) for fs in (8000, 16000, 24000, 32000, 44100, 48000) for us in (7500, 10000)]

# ---------------------------------------------------------------------------------------------------------------- float helpers
U = 2.0 ** -24  # unit roundoff of f32


def exp2_raw(x):
    """fast_math::exp2_raw, the decoder SNS's 2^x (decoder/spectral_noise_shaping.rs:122): SURVEY App. B.3, in f32 bit arithmetic.
    Part of the reference's definition (a true exp2 differs by about 1 %)."""
    x = np.asarray(x, np.float32)
    E = np.float32(1.1920929e-7)
    C0 = np.float32(np.float32(0.3371894346) * E) * E
    C1 = np.float32(0.657636276) * E
    C2 = np.float32(1.00172476)
    a = (np.float32(8388608.0) * x).astype(np.float64)
    mul = np.where(np.isnan(a), 0, np.clip(np.trunc(a), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)  # Rust `as i32`
    fl = (mul & 0xFF800000) - ((mul & 0x80000000) << 1)  # two's-complement AND: the floor to a multiple of 2^23
    frac = (mul - fl).astype(np.float32)
    approx = (C0 * frac + C1) * frac + C2
    bits = (approx.view(np.uint32).astype(np.int64) + fl) & 0xFFFFFFFF
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------- transforms
_mat = {}


def _cos(kind, n):
    key = (kind, n)
    if key not in _mat:
        k = np.arange(n, dtype=np.float64)[:, None] + 0.5
        if kind == "dct4":
            m = np.cos(np.pi / n * (np.arange(n, dtype=np.float64)[None, :] + 0.5) * k)
        else:  # "mdct": n x 2n, the LC3 MDCT kernel cos(pi/N (n + 1/2 + N/2)(k + 1/2))
            t = np.arange(2 * n, dtype=np.float64)[None, :] + 0.5 + n / 2.0
            m = np.sqrt(2.0 / n) * np.cos(np.pi / n * t * k)
        _mat[key] = m
    return _mat[key]


def dct4(x):
    """common/dct_iv.rs:49-66 (kissfft-based): y[k] = 2 sum_n x[n] cos(pi/N (n + 1/2)(k + 1/2)) -- the factor 2 is the
    reference's (`complex.r * 2.0`, :62-63), which with the MDCT's 1/sqrt(2N) (encoder/modified_dct.rs:101-104) gives the
    specification's sqrt(2/N)"""
    x = np.asarray(x, np.float64)
    return 2.0 * _cos("dct4", x.size) @ x


class Mdct:
    """encoder/modified_dct.rs:108-138: the low-delay MDCT over a time buffer t of 2N samples that carries from frame to frame:
    t = [last N - Z samples of the previous frame, this frame, Z zeros]; X[k] = sqrt(2/N) sum_n w[n] t[n] cos(pi/N (n + 1/2 + N/2)
    (k + 1/2)) (LC3 3.3.4)"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.prev = np.zeros(cfg.nf)

    def run(self, x):
        c = self.cfg
        t = np.concatenate([self.prev[c.z:], np.asarray(x, np.float64), np.zeros(c.z)])
        self.prev = np.asarray(x, np.float64).copy()
        return _cos("mdct", c.nf) @ (c.window * t)


def band_energies(cfg, X):
    """encoder/modified_dct.rs:140-152: E[b] = mean of X[k]^2 over band b (the reference sums x*x/width term by term, A14)"""
    b = cfg.bands
    return np.array([np.sum(np.square(X[b[i]:b[i + 1]])) / max(1, b[i + 1] - b[i]) for i in range(cfg.nb)])


def near_nyquist(cfg, eb):
    """encoder/modified_dct.rs:154-177 -> (flag, ratio of the upper bands' energy to 30 x the lower bands', or None above 32 kHz)"""
    if cfg.fs > 32000:
        return False, None
    idx = cfg.nb - 2 if cfg.ten_ms else cfg.nb - 4
    lo, hi = float(np.sum(eb[:idx])), float(np.sum(eb[idx:]))
    return hi > 30.0 * lo, (hi / (30.0 * lo) if lo > 0 else math.inf)


class Imdct:
    """decoder/modified_dct.rs:76-151: t[n] = sqrt(2/N) sum_k X[k] cos(pi/N (n + 1/2 + N/2)(k + 1/2)) over 2N samples (X zero above
    ne), windowed by w[2N - 1 - n]; low-delay overlap-add: out[n] = mem[n] + t[Z + n] for n < N - Z, out[N - Z + n] = t[N + n] for
    n < Z, and mem <- t[N + Z : 2N]"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.mem = np.zeros(cfg.nf - cfg.z)

    def run(self, spec):
        c = self.cfg
        X = np.zeros(c.nf)
        X[:c.ne] = np.asarray(spec, np.float64)[:c.ne]
        t = (_cos("mdct", c.nf).T @ X) * c.window[::-1]
        out = np.concatenate([self.mem + t[c.z:c.nf], t[c.nf:c.nf + c.z]])
        self.mem = t[c.nf + c.z:].copy()
        return out


# ---------------------------------------------------------------------------------------------------------------- encoder SNS
G_TILT = (14, 18, 22, 26, 30)  # encoder/spectral_noise_shaping.rs:214-219


def sns_scf(cfg, eb, attack, terms=False):
    """encoder/spectral_noise_shaping.rs:75-161,203-240 (LC3 3.3.7.2): the 16 unquantised scale factors from the band energies
    (terms: also the 16 downsampled log-energies before the mean removal, the scale of its rounding)"""
    eb = np.asarray(eb, np.float64)
    d = 64 - cfg.nb
    if d > 0:  # :75-90 the first d bands doubled, then the rest (8 kHz / 7.5 ms, nb = 60)
        e = np.concatenate([np.repeat(eb[:d], 2), eb[d:]])[:64]
    else:
        e = eb.copy()
    s = np.empty(64)  # :92-98 smoothing
    s[0] = 0.75 * e[0] + 0.25 * e[1]
    s[1:63] = 0.25 * e[:62] + 0.5 * e[1:63] + 0.25 * e[2:]
    s[63] = 0.25 * e[62] + 0.75 * e[63]
    s *= 10.0 ** (np.arange(64) * G_TILT[cfg.fs_ind] / 630.0)  # pre-emphasis
    floor = max(np.mean(s) * 1e-4, 2.0 ** -32)  # :221-228 noise floor
    s = np.maximum(s, floor)
    L = np.log2(1.1920929e-7 + s) / 2.0  # :230-233
    w = np.array([1, 2, 3, 3, 2, 1]) / 12.0  # :100-124 downsampling with the edges clamped
    Lp = np.concatenate([[L[0]], L, [L[63]]])
    ds = np.array([np.dot(w, Lp[4 * b:4 * b + 6]) for b in range(16)])
    t = ds
    ds = 0.85 * (ds - np.mean(ds))  # :126-132
    if attack:  # :134-161
        a = np.array([np.mean(ds[max(0, n - 2):min(16, n + 3)]) for n in range(16)])
        ds = (0.5 if cfg.ten_ms else 0.3) * (a - np.mean(a))
    return (ds, t) if terms else ds


def sns_scfq(cfg, ind_lf, ind_hf, y, g_ind, shape_j):
    """decoder/spectral_noise_shaping.rs:21-96 (LC3 3.4.7.3): the quantised scale factors from the SNS side information and the
    de-enumerated integer vector y (16 entries): st1 + G / |y| * D y"""
    T = tables()
    st1 = np.concatenate([T["LFCB"][ind_lf], T["HFCB"][ind_hf]])
    gains = (T["SNS_VQ_REG_ADJ_GAINS"], T["SNS_VQ_REG_LF_ADJ_GAINS"], T["SNS_VQ_NEAR_ADJ_GAINS"], T["SNS_VQ_FAR_ADJ_GAINS"])[shape_j]
    g = gains[g_ind & (len(gains) - 1)]
    y = np.asarray(y, np.float64)
    n = np.sqrt(np.dot(y, y))
    return st1 + (g / n if n else g) * (T["D"] @ y)


def sns_interp(cfg, scf, decoder):
    """16 -> 64 interpolation (encoder :163-183, decoder :65-96) and the nb = 60 reduction, which differs between the two sides
    (encoder i >= 4 -> sf[diff + 1], decoder sf[i + 4])"""
    scf = np.asarray(scf, np.float64)
    s = np.empty(64)
    s[0] = s[1] = scf[0]
    d = np.diff(scf)
    for j, f in enumerate((0.125, 0.375, 0.625, 0.875)):
        s[2 + j:62:4] = scf[:15] + f * d
    s[62] = scf[15] + 0.125 * (scf[15] - scf[14])
    s[63] = scf[15] + 0.375 * (scf[15] - scf[14])
    n2 = 64 - cfg.nb
    if n2:
        r = s.copy()
        r[:n2] = (s[0:2 * n2:2] + s[1:2 * n2:2]) / 2.0
        r[n2:cfg.nb] = s[n2 + 1] if not decoder else s[2 * n2:cfg.nb + n2]
        s = r
    return s[:cfg.nb]


def apply_bands(cfg, X, g):
    out = np.asarray(X, np.float64).copy()
    b = cfg.bands
    for i in range(cfg.nb):
        out[b[i]:b[i + 1]] *= g[i]
    return out


def sns_shape(cfg, X, scfq):
    """encoder/spectral_noise_shaping.rs:264-268: X[k] * 2^-scf_int[b] over band b"""
    return apply_bands(cfg, X, 2.0 ** -sns_interp(cfg, scfq, decoder=False))


def sns_decode(cfg, X, scfq):
    """decoder/spectral_noise_shaping.rs:113-127: X[k] * exp2_raw(scf_int[b]) (the reference's fast exp2, App. B.3)"""
    g = exp2_raw(sns_interp(cfg, scfq, decoder=True).astype(np.float32))
    return apply_bands(cfg, X, g)


# ---------------------------------------------------------------------------------------------------------------- TNS
def tns_rc(rc_i, decoder):
    """quantised reflection coefficients sin(pi/17 (i - 8)) (encoder/temporal_noise_shaping.rs:267-292, decoder :39-47); the decoder
    treats index 0 as unset, coefficient 0"""
    rc_i = np.asarray(rc_i, np.int64)
    rc = np.sin(np.pi / 17.0 * (rc_i - 8))
    if decoder:
        rc = np.where(rc_i == 0, 0.0, rc)
    return rc


def tns_analysis(cfg, X, p_bw, rc_order, rc_i):
    """encoder/temporal_noise_shaping.rs:313-340 (LC3 3.3.8.4): the FIR lattice f_k = f_(k-1) + r_k b_(k-1)[n-1],
    b_k = r_k f_(k-1) + b_(k-1)[n-1] over each filter's lines; one lattice state for both filters"""
    out = np.asarray(X, np.float64).copy()
    rc = tns_rc(rc_i, decoder=False)
    st = np.zeros(8)  # b_k[n-1], k = 0..7
    for f, (start, stop) in enumerate(cfg.tns_enc[p_bw]):
        order = int(rc_order[f])
        if not order:
            continue
        r = rc[8 * f:8 * f + order]
        for n in range(start, stop):
            fk = bk = out[n]
            nst = np.empty(order)
            for k in range(order):
                nst[k] = bk
                fk, bk = fk + r[k] * st[k], r[k] * fk + st[k]
            st[:order] = nst
            out[n] = fk
    return out


def tns_synthesis(cfg, X, p_bw, num_tns_filters, rc_order, rc_i):
    """decoder/temporal_noise_shaping.rs:24-137 (LC3 3.4.6): the all-pole lattice, the inverse of tns_analysis: from f_P = x,
    f_(k-1) = f_k - r_k b_(k-1)[n-1], b_k = r_k f_(k-1) + b_(k-1)[n-1], output f_0 = b_0"""
    out = np.asarray(X, np.float64).copy()
    rc = tns_rc(rc_i, decoder=True)
    st = np.zeros(8)
    for f, (start, stop) in enumerate(cfg.tns_dec[p_bw][:num_tns_filters]):
        order = int(rc_order[f])
        if not order:
            continue
        r = rc[8 * f:8 * f + order]
        for n in range(start, stop):
            fk = out[n]
            fs_ = np.empty(order + 1)
            fs_[order] = fk
            for k in range(order, 0, -1):
                fs_[k - 1] = fs_[k] - r[k - 1] * st[k - 1]
            nst = np.empty(order)
            nst[0] = fs_[0]
            for k in range(1, order):
                nst[k] = r[k - 1] * fs_[k - 1] + st[k - 1]
            st[:order] = nst
            out[n] = fs_[0]
    return out


# ---------------------------------------------------------------------------------------------------------- decoder spectrum
def noise_fill(cfg, X, x_int, is_zero_frame, seed, bandwidth, noise_factor):
    """decoder/noise_filling.rs:18-56 (LC3 3.4.4): lines k in [start, min(bw_stop, ne)) whose integer neighbourhood
    [k - w, min(bw_stop - 1, k + w)] is all zero get +-(8 - F) / 16, the sign from the 16-bit LCG seeded by the spectrum"""
    out = np.asarray(X, np.float64).copy()
    if is_zero_frame:
        return out
    bw_stop = cfg.nf_bw_stop[bandwidth]
    w = cfg.nf_width
    level = (8.0 - noise_factor) / 16.0
    nz = np.asarray(x_int) != 0
    s = int(seed)
    for k in range(cfg.nf_start, min(bw_stop, cfg.ne)):
        if not nz[k - w:min(bw_stop - 1, k + w) + 1].any():
            s = (13849 + s * 31821) & 0xFFFF
            out[k] = level if s < 0x8000 else -level
    return out


def global_gain(cfg, X, frame_num_bits, gg_ind):
    """decoder/global_gain.rs:15-25 (LC3 3.4.5): X * 10^((gg_ind + gg_off) / 28)"""
    f = cfg.fs_ind + 1
    gg_off = -min(115, frame_num_bits // (10 * f)) - 105 - 5 * f
    return np.asarray(X, np.float64) * 10.0 ** ((gg_ind + gg_off) / 28.0)


def residual(X, lsb_mode, bits):
    """decoder/residual_spectrum.rs:13-39: one residual bit per non-zero line in order: +-0.3125 / -+0.1875 (lsb_mode: none)"""
    out = np.asarray(X, np.float64).copy()
    if lsb_mode:
        return out
    nz = np.flatnonzero(out)[:len(bits)]
    b = np.asarray(bits[:nz.size], bool)
    pos = out[nz] > 0
    out[nz] += np.where(b, np.where(pos, 0.3125, 0.1875), np.where(pos, -0.1875, -0.3125))
    return out


# ---------------------------------------------------------------------------------------------------------------- LTPF
def ltpf_pitch(fs, pitch_index):
    """decoder/long_term_post_filter.rs:164-189: the pitch lag at the output rate, in quarter samples -> (integer, fraction)"""
    pi = int(pitch_index)
    if pi >= 440:
        p_i, p_fr = pi - 283, 0
    elif pi >= 380:
        p_i = pi // 2 - 63
        p_fr = 2 * pi - 4 * p_i - 252
    else:
        p_i = pi // 4 + 32
        p_fr = pi + 128 - 4 * p_i
    pitch_fs = (p_i + p_fr / 4.0) * (8000.0 * math.ceil(fs / 8000.0) / 12800.0)
    p_up = int(math.floor(pitch_fs * 4.0 + 0.5))
    return p_up // 4, p_up % 4


class Ltpf:
    """decoder/long_term_post_filter.rs (LC3 3.4.9): y[n] = x[n] - s(n) (sum_k c_num[k] x[n - k] - sum_k c_den[k] y[n - p + l_den/2 - k])
    over a linear history of x and y, with the five frame-to-frame transitions of :142-160 / :345-424: off-off (y = x), off-on (the
    new filter faded in over 2.5 ms, s = n / norm), on-off (the old filter faded out, s = 1 - n / norm), on-on with the same lag (the
    filter throughout), on-on with a new lag (old filter faded out, then the new one faded in on that output).  The reference keeps
    its history in a ring of num_mem_blocks frames indexed with a negative wrap only; a linear history equals it
    except for the longest lags at 10 ms (_filter).  Gains and taps: :142-160, 192-242 (A11: t_nbits >= 560 + 80 fs_ind -> gain 0; A9: 44.1 kHz keeps
    l_den = 11 and the first 10 / 12 taps of the 48 kHz tables)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.hist = 4 * cfg.nf
        self.x = np.zeros(self.hist)
        self.y = np.zeros(self.hist)
        self.active_prev = False
        self.p_mem = (0, 0)
        self.c_mem = (np.zeros(cfg.ltpf_l_den - 1), np.zeros(cfg.ltpf_l_den + 1))
        self.trans = None

    def coeffs(self, active, pitch_frac, nbits):
        c = self.cfg
        l_den = c.ltpf_l_den
        if not active:
            return np.zeros(l_den - 1), np.zeros(l_den + 1)
        t_nbits = nbits if c.ten_ms else int(math.floor(nbits * 10.0 / 7.5 + 0.5))
        sf = 80 * c.fs_ind
        gi = next((i for i, lim in enumerate((320, 400, 480, 560)) if t_nbits < lim + sf), None)
        gain = (0.4, 0.35, 0.3, 0.25)[gi] if gi is not None else 0.0
        gi = gi or 0
        return 0.85 * gain * c.ltpf_num[gi][:l_den - 1], gain * c.ltpf_den[pitch_frac][:l_den + 1]

    def _filter(self, xs, ys, i, cn, cd, p, written):
        """the filter term at history index i; ys is final below `written`.  The reference's output history is a ring of
        num_mem_blocks frames: a lag longer than the ring minus what this frame has already written reads the slot
        this frame has overwritten, i.e. the sample one ring length later.  That happens at 10 ms (a ring of two frames) for the
        longest lags, e.g. pitch index 511 (lag 855 at 48 kHz, 142 at 8 kHz) right after a change of lag (transition 5), whose
        first pass has overwritten the first 2.5 ms"""
        c = self.cfg
        ring = (2 if c.ten_ms else 3) * c.nf
        num = np.dot(cn, xs[i - np.arange(cn.size)])
        j = i - p + c.ltpf_l_den // 2 - np.arange(cd.size)
        j = np.where(j + ring < written, j + ring, j)
        den = np.dot(cd, ys[j])
        return num - den

    def run(self, x, active, pitch_index, nbits):
        c = self.cfg
        nf, H = c.nf, self.hist
        s25 = (48000 if c.fs == 44100 else c.fs) // 400
        norm = nf // 4 if c.ten_ms else nf // 3
        p, pfr = ltpf_pitch(c.fs, pitch_index) if active else (0, 0)
        cn, cd = self.coeffs(active, pfr, nbits)
        cn_old, cd_old = self.c_mem
        p_old = self.p_mem[0]
        xs = np.concatenate([self.x, np.asarray(x, np.float64)])
        ys = np.concatenate([self.y, np.zeros(nf)])
        if not active and not self.active_prev:
            trans = 1
        elif active and not self.active_prev:
            trans = 2
        elif not active:
            trans = 3
        elif (p, pfr) == self.p_mem:
            trans = 4
        else:
            trans = 5
        if trans == 1:
            ys[H:] = xs[H:]
        elif trans in (2, 4):
            for n in range(nf):
                fade = n / norm if (trans == 2 and n < s25) else 1.0
                ys[H + n] = xs[H + n] - fade * self._filter(xs, ys, H + n, cn, cd, p, H + n)
        else:
            for n in range(s25):  # the old filter faded out
                ys[H + n] = xs[H + n] - (1.0 - n / norm) * self._filter(xs, ys, H + n, cn_old, cd_old, p_old, H + n)
            if trans == 5:  # the new filter faded in on that output, then the new filter alone
                mid = ys.copy()
                for n in range(s25):
                    ys[H + n] = mid[H + n] - (n / norm) * self._filter(mid, ys, H + n, cn, cd, p, H + s25)
                for n in range(s25, nf):
                    ys[H + n] = xs[H + n] - self._filter(xs, ys, H + n, cn, cd, p, H + n)
            else:
                ys[H + s25:] = xs[H + s25:]
        self.x = xs[nf:]
        self.y = ys[nf:]
        self.active_prev = bool(active)
        self.p_mem = (p, pfr)
        self.c_mem = (cn, cd)
        self.trans = trans
        return ys[H:]


def output_pcm(x):
    """decoder/output_scaling.rs:13-25: round half away from zero, saturate to int16"""
    x = np.asarray(x, np.float64)
    return np.clip(np.trunc(x + np.copysign(0.5, x)), -32768, 32767).astype(np.int64)


# ------------------------------------------------------------------------------------------------------- encoder decisions
# encoder/bandwidth_detector.rs:5-18,64-127 (LC3 3.3.5): per candidate bandwidth, the bands whose mean energy is tested
BW_START_10 = ((53,), (47, 59), (44, 54, 60), (41, 51, 57, 61))
BW_STOP_10 = ((63,), (56, 63), (52, 59, 63), (49, 55, 60, 63))
BW_START_75 = ((51,), (45, 58), (42, 53, 60), (40, 51, 57, 61))
BW_STOP_75 = ((63,), (55, 63), (51, 58, 63), (48, 55, 60, 63))
BW_TQ, BW_TC = (20, 10, 10, 10), (15, 23, 20, 20)
BW_L_10, BW_L_75 = (4, 4, 3, 1), (4, 4, 3, 2)


def bandwidth(cfg, eb):
    """-> (bandwidth index, [(quantity, threshold) of every comparison the decision rests on])"""
    fsi = cfg.fs_ind
    if fsi == 0:
        return 0, []
    start = (BW_START_10 if cfg.ten_ms else BW_START_75)[fsi - 1]
    stop = (BW_STOP_10 if cfg.ten_ms else BW_STOP_75)[fsi - 1]
    L = (BW_L_10 if cfg.ten_ms else BW_L_75)
    eb = np.asarray(eb, np.float64)
    tests, bw = [], 0
    for k in range(fsi - 1, -1, -1):
        q = float(np.mean(eb[start[k]:stop[k] + 1]))
        tests.append((q, BW_TQ[k]))
        if q >= BW_TQ[k]:
            bw = k + 1
            break
    if bw == fsi:
        return bw, tests
    l = L[bw]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = eb[start[bw] + 1 - 2 * l:start[bw] - l] / eb[start[bw] + 1 - l:start[bw]]
        if cfg.spec_flags & SPEC_BW_CUTOFF_DB:
            r = 10.0 * np.log10(1.1920929e-7 + r)
    r = r[~np.isnan(r)]  # f32::max ignores NaN (A7)
    m = max(0.0, float(np.max(r))) if r.size else 0.0
    tests.append((m, BW_TC[bw]))
    return (bw if m > BW_TC[bw] else fsi), tests
