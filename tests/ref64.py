"""float64 references of the codec's float stages, written from their definitions (numpy only).

A second derivation, independent of the oracle (oracle/*.c) and of the device code (lc3-codec_amd/csrc/*.h): every stage below is
the formula of the stage, evaluated in float64 over whole vectors, not a transliteration of either restatement.  Each one cites the
reference (ninjasource/lc3-codec v0.2.0, src/) at the lines that define it, and follows the reference's deviations from the LC3
specification that touch it.  The only constants taken from the repository are the
tables of tables/lc3_tables.h, parsed here (the f32 bit patterns become float32 values, then float64).

The encoder's decisions are restated too (the last section): attack detector, TNS analysis, LTPF analysis, the rate loop (bit
budget, gain estimate and adjustment, quantisation, bit count), residual bits and noise level.  Each model returns, next to a
decision, its closest call (Calls): how near the float64 evaluation came to deciding otherwise, which is what tells a rounding
difference from a wrong constant (tests/ref64_check.py).

Integer stages are not restated: side information, the arithmetic decoder, MPVQ de-enumeration, the SNS vector search and the packer.
Their integer outputs are inputs here.

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


# encoder/temporal_noise_shaping.rs:119-200: the three sub-blocks of each filter's normalised autocorrelation
TNS_SUB_10 = ((((12, 34), (34, 57), (57, 80)),), (((12, 61), (61, 110), (110, 160)),), (((12, 88), (88, 164), (164, 240)),),
              (((12, 61), (61, 110), (110, 160)), ((160, 213), (213, 266), (266, 320))),
              (((12, 74), (74, 137), (137, 200)), ((200, 266), (266, 333), (333, 400))))
TNS_SUB_75 = ((((9, 26), (26, 43), (43, 60)),), (((9, 46), (46, 83), (83, 120)),), (((9, 66), (66, 123), (123, 180)),),
              (((9, 46), (46, 82), (82, 120)), ((120, 159), (159, 200), (200, 240))),
              (((9, 56), (56, 103), (103, 150)), ((150, 200), (200, 250), (250, 300))))
# encoder/spectral_quantization.rs:351-353
ADJ_T1, ADJ_T2, ADJ_T3 = (80, 230, 380, 530, 680), (500, 1025, 1550, 2075, 2600), (850, 1700, 2550, 3400, 4250)


def attack_window(fs, ten):
    """encoder/attack_detector.rs:91-105: the frame sizes (bytes) at which the detector runs"""
    if fs < 32000:
        return None
    if ten:
        return (81, 1 << 30) if fs == 32000 else (100, 1 << 30)
    return (61, 150) if fs == 32000 else (75, 150)


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
    # the encoder's decisions (the last section of this file); config() fills every one
    att_window: tuple = None  # (first, one past the last) frame size in bytes at which the attack detector runs; None: never
    att_factor: float = 8.5
    tns_sub: tuple = None  # per bandwidth index, per filter: the three (start, stop) autocorrelation sub-blocks
    tns_gain_thresh: float = 1.5
    ltpf_up: int = 0  # the resampler's up-sampling factor towards 192 kHz
    ltpf_resamp: float = 1.0  # its per-rate scale
    ltpf_len12: int = 128  # 12.8 kHz samples per frame
    ltpf_mmnc: bool = False  # the activation's extra term on the normalised correlation of two frames ago
    gg_off_rate: int = 1  # fs_ind + 1 in gg_off
    ari_const: tuple = (3, 4, 5)  # nbits_ari's constant by frame size
    ctx_half_strict: bool = True  # the bit count's context bit: n > ne / 2 (strict)
    q_offset: float = 0.375
    adj_t: tuple = (0, 0, 0)  # T1, T2, T3 of the gain adjustment at this rate
    tns_weight_bits: int = 480  # frames of fewer bits get the low-bitrate TNS weighting
    ltpf_gate: int = 560  # t_nbits (+ 80 fs_ind) from which the post-filter is never activated
    rate_flag_bits: int = 160  # frames of more bits (+ 160 fs_ind) count their spectrum with the high-rate contexts

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
               spec_flags=spec_flags, att_window=attack_window(fs, ten), tns_sub=TNS_SUB_10 if ten else TNS_SUB_75,
               ltpf_up=(24, 12, 8, 6, 4)[fs_ind], ltpf_resamp=0.5 if fs == 8000 else 1.0, ltpf_len12=128 if ten else 96,
               ltpf_mmnc=not ten, gg_off_rate=fs_ind + 1, adj_t=(ADJ_T1[fs_ind], ADJ_T2[fs_ind], ADJ_T3[fs_ind]),
               tns_weight_bits=480 if ten else 360)


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


# ------------------------------------------------------------------------------------------- encoder decisions: closest calls
class Calls:
    """the closest call of a decision: the smallest relative distance |lhs - rhs| / max(|lhs|, |rhs|) over the comparisons it went
    through.  Two values that are exactly equal in any precision (0 against 0) are no call at all."""

    def __init__(self):
        self.d = math.inf

    def note(self, lhs, rhs):
        lhs, rhs = float(lhs), float(rhs)
        m = max(abs(lhs), abs(rhs))
        if m > 0 and not (math.isnan(lhs) or math.isnan(rhs)):
            self.d = min(self.d, abs(lhs - rhs) / m)

    def gt(self, lhs, rhs):
        self.note(lhs, rhs)
        return lhs > rhs

    def lt(self, lhs, rhs):
        self.note(lhs, rhs)
        return lhs < rhs

    def to_int(self, x):
        """truncation towards zero of x >= 0; the call is x against the nearer integer"""
        self.note(x, math.floor(x + 0.5))
        return int(math.floor(x))

    def argmax(self, v, floor=None):
        """index of the first largest value (of the first that exceeds `floor`, else 0): best against second best, and the floor"""
        v = np.asarray(v, np.float64)
        i = int(np.argmax(v))
        if v.size > 1:
            rest = np.delete(v, i)
            self.note(v[i], float(np.max(rest)))
        if floor is not None:
            self.note(v[i], floor)
            if not v[i] > floor:
                return 0
        return i

    def merge(self, other):
        self.d = min(self.d, other.d)
        return self


# ---------------------------------------------------------------------------------------------------------- attack detector
def attack(cfg, x, nbytes, state, calls):
    """encoder/attack_detector.rs:45-128 (LC3 3.3.6).  state = (energy_last, max_energy_last, attack_pos_last, downsampled sample
    t-1, t-2) before the frame -> (flag, state after).  Outside the activity window the detector only clears its envelope."""
    e_last, max_last, pos_last, tm1, tm2 = state
    w = cfg.att_window
    if w is None or not (w[0] <= nbytes < w[1]):
        return False, (0.0, 0.0, -1, tm1, tm2)
    nd, nblk, limit = (160, 4, 2) if cfg.ten_ms else (120, 3, 1)
    d = np.asarray(x, np.int64).reshape(nd, cfg.nf // nd).sum(axis=1)  # :107-116 block sums
    ext = np.concatenate([[tm2, tm1], d]).astype(np.float64)
    hp = 0.375 * ext[2:] - 0.5 * ext[1:-1] + 0.125 * ext[:-2]  # :118-128
    pos = -1
    for n in range(nblk):
        energy = float(np.sum(np.square(hp[40 * n:40 * n + 40])))
        max_energy = max(0.25 * max_last, e_last)
        if calls.gt(energy, cfg.att_factor * max_energy):
            pos = n
        e_last, max_last = energy, max_energy
    return (pos >= 0 or pos_last >= limit), (e_last, max_last, pos, int(d[-1]), int(d[-2]))


# ---------------------------------------------------------------------------------------------------------------- TNS analysis
def tns_decide(cfg, S, p_bw, nbits, near_nyquist, calls):
    """encoder/temporal_noise_shaping.rs:40-64,80-115,204-292 (LC3 3.3.8.2-3): per filter, the normalised autocorrelation over
    three sub-blocks under the lag window exp(-(0.02 pi k)^2 / 2), Levinson-Durbin, the prediction-gain test, the low-bitrate
    weighting, and the quantisation of the reflection coefficients to pi / 17 steps of their arcsine -> (orders[2], rc_i[16])"""
    S = np.asarray(S, np.float64)
    weighting = nbits < cfg.tns_weight_bits  # :49-53
    lagw = np.exp(-0.5 * np.square(0.02 * np.pi * np.arange(9)))  # :81-84
    rc_i = np.full(16, 8, np.int64)
    orders = [0, 0]
    for f, subs in enumerate(cfg.tns_sub[p_bw]):
        es = [float(np.sum(np.square(S[a:b]))) for a, b in subs]
        if np.prod(es) == 0.0:  # :111
            r = np.zeros(9)
            r[0] = 3.0
        else:
            r = np.array([sum(float(np.dot(S[a:b - k], S[a + k:b])) / e for (a, b), e in zip(subs, es)) for k in range(9)])
        r = r * lagw
        a = np.zeros(9)
        a[0] = 1.0
        err = r[0]
        for k in range(1, 9):  # :213-232
            rc = -float(np.dot(a[:k], r[k:0:-1]))
            if err != 0.0:
                rc /= err
            nxt = a.copy()
            nxt[1:k] = a[1:k] + rc * a[k - 1:0:-1]
            nxt[k] = rc
            a = nxt
            err *= 1.0 - rc * rc
        gain = r[0] if err == 0.0 else r[0] / err
        if not (calls.gt(gain, cfg.tns_gain_thresh) and not near_nyquist):
            continue
        gamma = 1.0
        if weighting and gain < 2.0:  # :238-242 (continuous at 2: no call)
            gamma -= (1.0 - 0.85) * (2.0 - gain) / (2.0 - cfg.tns_gain_thresh)
        a = a * gamma ** np.arange(9)
        rcs = np.zeros(8)
        for k in range(8, 0, -1):  # :249-257 LPC -> reflection coefficients
            rcs[k - 1] = a[k]
            e = 1.0 - a[k] * a[k]
            nxt = a.copy()
            nxt[1:k] = (a[1:k] - a[k] * a[k - 1:0:-1]) / e
            a = nxt
        for k in range(8):  # :267-274, 343-349: round half away from zero
            q = math.asin(rcs[k]) / (math.pi / 17.0)
            rc_i[8 * f + k] = int(math.copysign(calls.to_int(abs(q) + 0.5), q)) + 8
        nz = np.flatnonzero(rc_i[8 * f:8 * f + 8] != 8)
        orders[f] = int(nz[-1]) + 1 if nz.size else 0  # :277-281
    return orders, rc_i


def tns_nbits(cfg, nbits, orders, rc_i, n_filters):
    """encoder/temporal_noise_shaping.rs:294-311: in integers"""
    T = tables()
    w = int(nbits < cfg.tns_weight_bits)
    total = 0
    for f in range(n_filters):
        o = int(orders[f])
        bits = 2048 + (int(T["AC_TNS_ORDER_BITS"][w][o - 1]) if o else 0)
        bits += sum(int(T["AC_TNS_COEF_BITS"][k][int(rc_i[8 * f + k])]) for k in range(o))
        total += (bits + 2047) // 2048
    return total


# --------------------------------------------------------------------------------------------------------------- LTPF analysis
class LtpfAnalysis:
    """encoder/long_term_post_filter.rs:139-469 (LC3 3.3.9): the input resampled to 12.8 kHz, high-passed at 50 Hz, decimated to
    6.4 kHz; the pitch lag from the weighted autocorrelation and from the neighbourhood of the last lag; its refinement at
    12.8 kHz to a quarter sample; the normalised correlation nc at that lag and the activation hysteresis on it.  All state is
    carried here in float64."""
    NMEM, K_MIN, K_MAX = 232, 17, 114

    def __init__(self, cfg):
        self.cfg = cfg
        self.len12 = cfg.ltpf_len12
        self.len6 = self.len12 // 2
        self.delay = 24 if cfg.ten_ms else 44
        self.ns = 240 // cfg.ltpf_up
        self.xs = np.zeros(self.ns + cfg.nf)
        self.x12 = np.zeros(self.len12 + self.delay + self.NMEM)
        self.x6 = np.zeros(64 + self.K_MAX)
        self.h1 = self.h2 = 0.0
        self.t_prev = self.K_MIN
        self.mem_pitch = 0.0
        self.mem_active = False
        self.mem_nc = self.mem_mem_nc = 0.0
        self.lags = (0, 0)

    def run(self, x, near_nyquist, nbits, pitch_calls, active_calls):
        """-> (pitch_index, pitch_present, ltpf_active); pitch_int of the frame is left in self.pitch_int"""
        c, T = self.cfg, tables()
        len12, len6, M = self.len12, self.len6, self.NMEM
        t_nbits = nbits if c.ten_ms else int(math.floor(nbits * 10.0 / 7.5 + 0.5))  # :142-146
        gain_on = self.gain_on = t_nbits < c.ltpf_gate + c.fs_ind * 80
        self.xs[:self.ns] = self.xs[-self.ns:].copy()  # :217-229
        self.xs[self.ns:] = np.asarray(x, np.float64)
        self.x12[:-len12] = self.x12[len12:].copy()
        self.x6[:-len6] = self.x6[len6:].copy()
        # :152-166 x12[n] = p f sum_k x[15 n / p + k - 120 / p] h[p k - 15 n mod p], |p k - 15 n mod p| < 120
        p, h = c.ltpf_up, T["TAB_RESAMP_FILTER"]
        new = np.zeros(len12)
        ks = np.arange(-(120 // p), 120 // p + 1)
        src = np.concatenate([self.xs, np.zeros(512)])  # (zeros past the frame: only a wrong len12 reads them)
        for n in range(len12):
            ih = p * ks - (15 * n) % p
            ok = (ih > -120) & (ih < 120)
            new[n] = np.dot(src[120 // p + (15 * n) // p + ks[ok]], h[119 + ih[ok]])
        new *= p * c.ltpf_resamp
        for n in range(len12):  # :169-177 the 50 Hz high-pass (direct form II)
            h50 = new[n] + 1.9652933726226904 * self.h1 - 0.9658854605688177 * self.h2
            new[n] = 0.9827947082978771 * h50 - 1.965589416595754 * self.h1 + 0.9827947082978771 * self.h2
            self.h2, self.h1 = self.h1, h50
        self.x12[self.delay + M:] = new
        t_cur, present = self._pitch(pitch_calls)
        index, p_int, p_fr = self._lag(t_cur, pitch_calls)
        active, nc, pitch = self._activation(p_int, p_fr, near_nyquist, gain_on, active_calls)
        self.pitch_int = p_int
        self.t_prev = t_cur  # :197-207
        self.mem_mem_nc = self.mem_nc
        if present:
            self.mem_pitch, self.mem_active, self.mem_nc = pitch, active, nc
        else:
            self.mem_pitch, self.mem_active, self.mem_nc = 0.0, False, 0.0
        return (index if present else 0), present, active

    def _pitch(self, calls):
        """:232-290"""
        len6, KMIN, KMAX = self.len6, self.K_MIN, self.K_MAX
        taps = (0.1236796411180537, 0.2353512128364889, 0.2819382920909148, 0.2353512128364889, 0.1236796411180537)
        src = self.x12[self.NMEM - 3:]
        self.x6[KMAX:KMAX + len6] = sum(t * src[i:i + 2 * len6:2] for i, t in enumerate(taps))
        cur = self.x6[KMAX:KMAX + len6]
        r = np.array([np.dot(cur, self.x6[KMAX - lag:KMAX - lag + len6]) for lag in range(KMIN, KMAX + 1)])
        rw = r * (1.0 - 0.5 * np.arange(r.size) / (KMAX - KMIN))
        t1 = calls.argmax(rw) + KMIN
        k0, k1 = max(KMIN, self.t_prev - 4) - KMIN, min(KMAX, self.t_prev + 4) - KMIN + 1
        t2 = calls.argmax(r[k0:k1]) + k0 + KMIN
        self.lags = (t1, t2)

        def norm(lag):
            return float(np.sum(np.square(self.x6[KMAX - lag:KMAX - lag + len6])))

        def ncorr(lag):
            with np.errstate(divide="ignore", invalid="ignore"):
                v = np.float64(r[lag - KMIN]) / np.sqrt(np.float64(norm(0) * norm(lag)))
            return 0.0 if math.isnan(v) else max(0.0, float(v))  # (f32::max drops the NaN of silence)

        nc1 = ncorr(t1)
        if t1 == t2:
            return t1, calls.gt(nc1, 0.6)  # (nc2 = nc1: the 0.85 test is nc1 > 0, exact)
        nc2 = ncorr(t2)
        if calls.gt(nc2, 0.85 * nc1):
            return t2, calls.gt(nc2, 0.6)
        return t1, calls.gt(nc1, 0.6)

    def _lag(self, t, calls):
        """:292-363 -> (pitch_index, pitch_int, pitch_fr)"""
        T, M, len12 = tables(), self.NMEM, self.len12
        k_min, k_max = max(32, 2 * t - 4), min(228, 2 * t + 4)
        cur = self.x12[M:M + len12]
        lo = k_min - 4
        corr = np.array([np.dot(cur, self.x12[M - k:M + len12 - k]) for k in range(lo, k_max + 5)])
        inner = corr[4:4 + k_max - k_min + 1]
        best = int(np.argmax(inner))
        p_int = k_min + best if inner[best] > 0.0 else k_min
        calls.argmax(inner, floor=0.0)
        rel = p_int - lo
        R_ = T["TAB_LTPF_INTERP_R"]

        def interp(d):
            return sum(corr[rel + m] * R_[4 * m - d + 15] for m in range(-4, 5) if -16 < 4 * m - d < 16)

        self.cls = 0 if p_int == 32 else 1 if p_int < 127 else 2 if p_int < 157 else 3
        ds = ([0, 1, 2, 3], [-3, -2, -1, 0, 1, 2, 3], [-2, 0, 2], [])[self.cls]
        p_fr = 0
        if ds:
            v = [interp(d) for d in ds]
            i = int(np.argmax(v))
            calls.argmax(v, floor=0.0)
            p_fr = ds[i] if v[i] > 0.0 else 0
        if p_fr < 0:
            p_int -= 1
            p_fr += 4
        if p_int < 127:
            index = 4 * p_int + p_fr - 128
        elif p_int < 157:
            index = 2 * p_int + p_fr // 2 - 126
        else:
            index = p_int + 283
        return index, p_int, p_fr

    def _activation(self, p_int, p_fr, near_nyquist, gain_on, calls):
        """:365-424"""
        c, T, M, len12 = self.cfg, tables(), self.NMEM, self.len12
        hx = T["TAB_LTPF_INTERP_X12K8"]

        def xi(shift, d):
            return sum(self.x12[M + shift - k:M + shift - k + len12] * hx[4 * k - d + 7] for k in range(-2, 3) if -8 < 4 * k - d < 8)

        a, b = xi(0, 0), xi(-p_int, p_fr)
        den = math.sqrt(float(np.dot(a, a)) * float(np.dot(b, b)))
        nc = float(np.dot(a, b)) / den if den > 0.0 else 0.0
        pitch = p_int + p_fr / 4.0
        active = False
        if gain_on and not near_nyquist:  # :394-406
            if not self.mem_active:
                active = ((not c.ltpf_mmnc or calls.gt(self.mem_mem_nc, 0.94)) and calls.gt(self.mem_nc, 0.94)
                          and calls.gt(nc, 0.94))
            else:
                active = calls.gt(nc, 0.9) or (abs(pitch - self.mem_pitch) < 2.0 and calls.gt(nc - self.mem_nc, -0.1)
                                               and calls.gt(nc, 0.84))
        return active, nc, pitch


# ------------------------------------------------------------------------------------------------------------------ rate loop
def bit_budget(cfg, nbits, nbits_bw, nbits_tns, nbits_ltpf):
    """encoder/spectral_quantization.rs:122-134"""
    ari = int(math.ceil(math.log2(cfg.ne / 2.0))) + (cfg.ari_const[0] if nbits <= 1280 else cfg.ari_const[1] if nbits <= 2560
                                                      else cfg.ari_const[2])
    return nbits - (nbits_bw + nbits_tns + nbits_ltpf + 38 + 8 + 3 + ari)


def gg_offset(cfg, nbits):
    """:165"""
    return -min(115, nbits // (10 * cfg.gg_off_rate)) - 105 - 5 * cfg.gg_off_rate


def bit_count(cfg, xq, nbits, nbits_spec):
    """:265-348, in integers (1/2048 bit units) -> dict(rate_flag, mode_flag, lastnz, lastnz_trunc, nbits_est, nbits_trunc,
    nbits_lsb)"""
    T = tables()
    look, bits = T["AC_SPEC_LOOKUP"], T["AC_SPEC_BITS"]
    ne = cfg.ne
    xq = [int(v) for v in xq]
    rate_flag = 512 if nbits > cfg.rate_flag_bits + cfg.fs_ind * 160 else 0
    mode_flag = nbits >= 480 + cfg.fs_ind * 160
    lastnz = ne
    while lastnz > 2 and xq[lastnz - 1] == 0 and xq[lastnz - 2] == 0:
        lastnz -= 2
    est = trunc = lsb = ctx = 0
    lastnz_trunc = 2
    for n in range(0, lastnz, 2):
        t = ctx + rate_flag
        if (n > ne // 2) if cfg.ctx_half_strict else (n >= ne // 2):
            t += 256
        a, b = abs(xq[n]), abs(xq[n + 1])
        a_lsb, b_lsb = a, b
        lev = 0
        while max(a, b) >= 4:
            est += int(bits[look[t + lev * 1024]][16])
            if lev == 0 and mode_flag:
                lsb += 2
            else:
                est += 2 * 2048
            a >>= 1
            b >>= 1
            lev = min(3, lev + 1)
        est += int(bits[look[t + lev * 1024]][a + 4 * b])
        est += 2048 * ((a_lsb > 0) + (b_lsb > 0))
        if lev > 0 and mode_flag:
            lsb += int(a_lsb >> 1 == 0 and xq[n] != 0) + int(b_lsb >> 1 == 0 and xq[n + 1] != 0)
        if (xq[n] != 0 or xq[n + 1] != 0) and (est + 2047) // 2048 <= nbits_spec:
            lastnz_trunc = n + 2
            trunc = est
        t = 1 + (a + b) * (lev + 1) if lev <= 1 else 12 + lev
        ctx = (ctx & 15) * 16 + t
    return dict(rate_flag=rate_flag, mode_flag=mode_flag, lastnz=lastnz, lastnz_trunc=lastnz_trunc,
                nbits_est=(est + 2047) // 2048 + lsb, nbits_trunc=(trunc + 2047) // 2048, nbits_lsb=lsb)


def global_gain_value(cfg, nbits, gg_ind):
    """:239"""
    return 10.0 ** ((gg_ind + gg_offset(cfg, nbits)) / 28.0)


def quantise(cfg, X, gg):
    """:240-246: sign(X) trunc(|X| / gg + 0.375) -> (integers, per line the relative distance of |X| / gg + 0.375 from the nearer
    integer: the line's closest call)"""
    y = np.abs(np.asarray(X, np.float64)) / gg + cfg.q_offset
    q = np.floor(y)
    near = np.floor(y + 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        call = np.where(np.maximum(y, near) > 0, np.abs(y - near) / np.maximum(y, near), np.inf)
    return (np.sign(X) * np.clip(q, 0, 32767)).astype(np.int64), call


class RateLoop:
    """encoder/spectral_quantization.rs:75-395 (LC3 3.3.10): the gain index by bisection on an estimate of the bits that the
    energies of four lines each would cost, limited by gg_min; one quantisation and bit count; one adjustment of the index by the
    miss.  State: nbits_offset_old, nbits_est_old, reset_offset_old -- and nbits_spec_old, which the reference never updates
    (SURVEY A1): it stays 0."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.reset_old = False
        self.offset_old = 0.0
        self.spec_old = 0
        self.est_old = 0

    def run(self, X, nbits, nbits_spec, calls):
        """-> (final gg_ind, dict of what the frame went through)"""
        c = self.cfg
        X = np.asarray(X, np.float64)
        if self.reset_old:  # :156-172
            offset = 0.0
        else:
            offset = 0.8 * self.offset_old + 0.2 * min(40.0, max(-40.0, self.offset_old + self.spec_old - self.est_old))
        spec_adj = calls.to_int(max(0.0, nbits_spec + offset + 0.5))
        gg_off = gg_offset(c, nbits)
        e = 10.0 * np.log10(2.0 ** -23 + np.sum(np.square(X.reshape(-1, 4)), axis=1))  # :390-395
        e = e[::-1] * 1.4
        fac, ind = 256, 255
        for _ in range(8):  # :174-209
            fac >>= 1
            ind -= fac
            g = float(ind + gg_off)
            tmp, zero = 0.0, True
            for v in e:
                if calls.lt(v, g):
                    if not zero:
                        tmp += 2.7 * 1.4
                else:
                    if calls.lt(g, v - 43.0 * 1.4):
                        tmp += 2.0 * v - 2.0 * g - 36.0 * 1.4
                    else:
                        tmp += v - g + 7.0 * 1.4
                    zero = False
            if calls.gt(tmp, spec_adj * 1.4 * 1.4) and not zero:
                ind += fac
        x_max = float(np.max(np.abs(X)))  # :212-228
        if x_max > 0.0:
            v = 28.0 * math.log10(x_max / (32768.0 - 0.375))
            calls.note(v, math.floor(v + 0.5))
            gg_min = int(math.ceil(v)) - gg_off
        else:
            gg_min = 0
        reset = ind < gg_min or x_max == 0.0
        if reset:
            ind = gg_min
        first = ind
        xq, line_calls = quantise(c, X, global_gain_value(c, nbits, ind))
        calls.d = min(calls.d, float(np.min(line_calls)))  # a line that lands on the other side changes the bit count
        bc = bit_count(c, xq, nbits, nbits_spec)
        est = bc["nbits_est"]
        self.offset_old, self.est_old, self.reset_old = offset, est, reset  # :97-100 after the first pass; nbits_spec_old: never
        t1, t2, t3 = c.adj_t  # :350-388
        if est < t1:
            delta = (est + 48.0) / 16.0
        elif est < t2:
            tmp1, tmp2 = t1 / 16.0 + 3.0, t2 / 48.0
            delta = (est - t1) * (tmp2 - tmp1) / (t2 - t1) + tmp1
        elif est < t3:
            delta = est / 48.0
        else:
            delta = t3 / 48.0
        delta = float(calls.to_int(delta + 0.5))
        delta2 = delta + 2.0
        branch = 0
        if (ind < 255 and est > nbits_spec) or (ind > 0 and est < nbits_spec - delta2):
            if est < nbits_spec - delta2:
                ind, branch = ind - 1, -1
            elif ind == 254 or est < nbits_spec + delta:
                ind, branch = ind + 1, 1
            else:
                ind, branch = ind + 2, 2
            ind = max(ind, gg_min)
        return ind, dict(first=first, gg_min=gg_min, limited=bool(reset and x_max > 0.0), silent=x_max == 0.0,
                         branch=branch if ind != first else 0, nbits_est=est)


def ac_finish_short(cfg, nbits, orders, rc_i, xq, lastnz_trunc):
    """encoder/bitstream_encoding.rs:224-326,354-374,417-429, in integers: the range coder's (low, range) after the TNS symbols and
    the spectrum's, and whether its finish then leaves the codeword one bit short.  The finish picks the shortest
    `val` with [val, val + mask] inside [low, low + range); where low + mask and low + range have both passed 2^24 it compares
    val + mask with the UNMASKED low + range, which then always looks large enough, so that the extra bit the test is there to add
    is never taken: -> True when the masked comparison would have taken it.  Such a codeword reaches past the interval's end,
    and the bits that follow it in the frame can carry the decoder's value into the next symbol's interval: the last coded pair
    then decodes as another."""
    T = tables()
    low, rng = 0, 0x00FFFFFF

    def encode(cum, freq):
        nonlocal low, rng
        r = rng >> 10
        low = (low + r * int(cum)) & 0x00FFFFFF
        rng = r * int(freq)
        while rng < 0x10000:
            rng <<= 8
            low = (low << 8) & 0x00FFFFFF

    w = int(nbits < cfg.tns_weight_bits)
    for f in (0, 1):
        o = int(orders[f])
        if o > 0:
            encode(T["AC_TNS_ORDER_CUMFREQ"][w][o - 1], T["AC_TNS_ORDER_FREQ"][w][o - 1])
            for k in range(o):
                encode(T["AC_TNS_COEF_CUMFREQ"][k][int(rc_i[8 * f + k])], T["AC_TNS_COEF_FREQ"][k][int(rc_i[8 * f + k])])
    look, cum, freq = T["AC_SPEC_LOOKUP"], T["AC_SPEC_CUMFREQ"], T["AC_SPEC_FREQ"]
    rate_flag = 512 if nbits > cfg.rate_flag_bits + cfg.fs_ind * 160 else 0
    ctx = 0
    for n in range(0, lastnz_trunc, 2):
        t = ctx + rate_flag + (256 if n > cfg.ne // 2 else 0)
        a, b = abs(int(xq[n])), abs(int(xq[n + 1]))
        lev = 0
        while max(a, b) >= 4:
            pki = look[t + min(lev, 3) * 1024]
            encode(cum[pki][16], freq[pki][16])
            a >>= 1
            b >>= 1
            lev += 1
        pki = look[t + min(lev, 3) * 1024]
        encode(cum[pki][a + 4 * b], freq[pki][a + 4 * b])
        lev = min(lev, 3)
        t = 1 + (a + b) * (lev + 1) if lev <= 1 else 12 + lev
        ctx = (ctx & 15) * 16 + t
    bits = 1
    while (rng >> (24 - bits)) == 0:
        bits += 1
    mask = 0x00FFFFFF >> bits
    val = low + mask
    over1, high = val >> 24, low + rng
    val &= 0x00FFFFFF & ~mask
    return over1 == 1 and high >> 24 == 1 and val + mask >= (high & 0x00FFFFFF)


def residual_bits(X, xq, gg, n_max):
    """encoder/residual_spectrum.rs:42-58: one bit per non-zero line, X >= x_q gg -> (bits, per bit the relative distance)"""
    X = np.asarray(X, np.float64)
    k = np.flatnonzero(xq)[:max(0, n_max)]
    rhs = np.asarray(xq, np.float64)[k] * gg
    call = np.abs(X[k] - rhs) / np.maximum(np.abs(X[k]), np.abs(rhs))
    return (X[k] >= rhs).astype(np.uint8), call


def noise_factor(cfg, X, xq, bw, gg, calls):
    """encoder/noise_level_estimation.rs:21-55 (LC3 3.3.12): 8 - 16 x the mean of |X| / gg over the lines from nf_start below the
    bandwidth's stop whose neighbourhood of +-nf_width lines quantised to zero, rounded and limited to 0 .. 7"""
    bw_stop, w = cfg.nf_bw_stop[bw], cfg.nf_width
    nz = np.asarray(xq) != 0
    ks = [k for k in range(cfg.nf_start, min(cfg.ne, bw_stop)) if not nz[k - w:min(bw_stop, k + w + 1)].any()]
    level = float(np.mean(np.abs(np.asarray(X, np.float64)[ks]) / gg)) if ks else 0.0
    v = 8.0 - 16.0 * level + 0.5
    for b in range(1, 8):  # the steps of min(7, trunc(v)); below 1 every value gives 0
        calls.note(v, float(b))
    return min(7, int(v)) if v >= 0.5 else 0
