"""Frames with chosen contents, written by the oracle's bitstream writer (lc3o_kat_bitstream, oracle/lc3_kat.c): every field of an LC3
frame set by the caller instead of by an encoder, so that the decoder and lc3gpu_inspect can be held to the parts of the format the
project's own encoder never writes.  compose() writes one frame; rewrite() parses a real frame with the oracle's two parser stages,
changes fields and writes it again, which keeps real spectra under chosen side information.  Test infrastructure only."""
import ctypes
import functools

import numpy as np

import inspect_lib as I
import oracle_lib as O

NBITS_BW = [0, 1, 2, 2, 3]  # per fs_ind (oracle/lc3_enc.c: lc3o_enc_bandwidth)
SNS_GAINS = [2, 4, 4, 8]  # gain indices per shape (side information: 1, 2, 2 and 3 bits)
M10 = 2390004  # size of the 10-dimensional, 10-pulse MPVQ: the joint index's radix (oracle/lc3_enc.c: lc3o_enc_sns_quant_spec)
FAR_BASE = 15158272  # joint-index base of shape 3


def fs_index(fs):
    return {8000: 0, 16000: 1, 24000: 2, 32000: 3, 44100: 4, 48000: 4}[fs]


def derived(fs, us, nbytes):
    """(nbits_bw, rate_flag, lpc_weighting) as the oracle encoder derives them from configuration and frame size"""
    nbits, fi = 8 * nbytes, fs_index(fs)
    return NBITS_BW[fi], 512 if nbits > 160 + fi * 160 else 0, int(nbits < (480 if us == 10000 else 360))


def sns_joint(shape, gind, idx_a, ls_indb=0, idx_b=0):
    """the joint index of the SNS second stage, by the oracle encoder's formula (oracle/lc3_enc.c, the switch on shape_j)"""
    if shape == 0:
        return (2 * idx_b + ls_indb + 2) * M10 + idx_a
    if shape == 1:
        return (gind & 1) * M10 + idx_a
    if shape == 2:
        return idx_a
    return FAR_BASE + (gind & 1) + 2 * idx_a


def sns(ind_lf=0, ind_hf=0, shape=0, gind=0, ls_inda=0, idx_a=0, ls_indb=0, idx_b=0):
    return dict(ind_lf=ind_lf, ind_hf=ind_hf, shape=shape, gind=gind, ls_inda=ls_inda, idx_a=idx_a, ls_indb=ls_indb, idx_b=idx_b)


def compose(fs, us, nbytes, x_q=(), bw=None, lastnz=None, lsb_mode=0, gg_ind=128, tns_orders=(0, 0), rc_i=None, pitch_present=0, ltpf_active=0,
            pitch_index=0, sns_vq=None, noise_factor=0, res_bits=()):
    """one frame of nbytes bytes.  bw None: the largest index of the rate; lastnz None: the smallest even count that holds x_q's non-zero
    lines (2 for an all-zero spectrum); rc_i: up to 16 values, filter 1's from position 8 on; sns_vq: sns(...)"""
    cfg = I.config(fs, us)
    nbits_bw, rate_flag, weighting = derived(fs, us, nbytes)
    bw = cfg.fs_ind if bw is None else bw
    x = np.zeros(400, np.int16)
    x[:len(x_q)] = np.asarray(x_q, np.int16)
    if lastnz is None:
        nz = np.nonzero(x)[0]
        lastnz = 2 if len(nz) == 0 else int(nz[-1]) // 2 * 2 + 2
    assert lastnz % 2 == 0 and 2 <= lastnz
    q = dict(sns())
    q.update(sns_vq or {})
    flat = np.array([q["ind_lf"], q["ind_hf"], q["shape"], q["gind"], q["ls_inda"],
                     sns_joint(q["shape"], q["gind"], q["idx_a"], q["ls_indb"], q["idx_b"])], np.int64)
    orders = np.array(list(tns_orders) + [0, 0], np.int32)[:2]
    rc = np.full(16, 8, np.int32)
    if rc_i is not None:
        rc[:len(rc_i)] = rc_i
    res = np.ascontiguousarray(list(res_bits) + [0], np.uint8)
    out = np.zeros(nbytes, np.uint8)
    O.lib().lc3o_kat_bitstream(fs, us, int(bw), nbits_bw, int(lastnz), int(lsb_mode), int(gg_ind), 1 if bw < 3 else 2, O.P(orders), O.P(rc), weighting,
                               int(pitch_present), int(ltpf_active), int(pitch_index), O.P(flat), int(noise_factor), rate_flag, 0, O.P(x), O.P(res),
                               len(res_bits), O.P(out), nbytes)
    return out


def parse(fs, us, frame):
    """the frame's record as lc3gpu_inspect writes it (inspect_lib.OracleInspector): word 0 is the status"""
    return I.OracleInspector(fs, us).record(np.asarray(frame, np.uint8))


def parse_full(fs, us, frame):
    """(status, fields) from lc3o_dec_side_info + lc3o_dec_arith: fields holds what compose() takes, so that compose(fs, us, len(frame),
    **fields) writes the frame again"""
    ins = I.OracleInspector(fs, us)
    rec = ins.record(np.asarray(frame, np.uint8))
    if rec[0]:
        return int(rec[0]), None
    w = rec[2:22]
    a = ins.ad
    shape = 2 * int(w[14]) + int(w[13])
    fields = dict(x_q=np.array(ins.x[:], np.int64), bw=int(w[0]), lastnz=int(w[1]), lsb_mode=int(w[2]), gg_ind=int(w[3]),
                  tns_orders=(int(a.rc_order[0]), int(a.rc_order[1])), rc_i=[int(v) for v in a.rc_i], pitch_present=int(w[16]), ltpf_active=int(w[17]),
                  pitch_index=int(w[18]), noise_factor=int(w[19]),
                  sns_vq=sns(int(w[7]), int(w[8]), shape, int(w[15]), int(w[9]), int(w[11]) & 0xFFFFFFFF, int(w[10]), int(w[12]) & 0xFFFFFFFF),
                  res_bits=[int(b) for b in a.residual_bits[:a.n_residual_bits]])
    return 0, fields


def rewrite(fs, us, frame, nbytes=None, **changes):
    """a real frame with some fields changed: parsed by the oracle, written again at the same size, or at nbytes (the global gain's
    offset follows the size, so the level moves with it; the spectrum's shape does not).  lsb_mode = 0 frames only (in lsb mode the
    parser folds the lsb bits into the spectrum, which the writer would have to take apart again).  The changed frame must still parse: the
    frame needs enough slack for what the change adds (residual bits are given up first)."""
    st, f = parse_full(fs, us, frame)
    assert st == 0 and f["lsb_mode"] == 0, "rewrite() takes a clean lsb_mode = 0 frame"
    assert np.abs(f["x_q"]).max() <= 32767
    f.update(changes)
    nbytes = len(frame) if nbytes is None else nbytes
    out = compose(fs, us, nbytes, **f)
    assert parse(fs, us, out)[0] == 0, "the rewritten frame does not parse: not enough slack at %d bytes" % nbytes
    return out


@functools.lru_cache(None)
def sns_index_limits():
    """per shape the largest valid idx_a, and for shape 0 the largest (idx_b, ls_indb) beside it -- asked of the oracle's parser by
    bisection: an index is valid when a frame carrying it parses and the parser hands back the same shape, gain and index.
    -> {shape: idx_a_max}, (idx_b_max, ls_indb_max)"""
    fs, us, n = 48000, 10000, 60

    def valid(shape, idx_a, ls_indb=0, idx_b=0):
        g = SNS_GAINS[shape] - 1
        st, f = parse_full(fs, us, compose(fs, us, n, sns_vq=sns(3, 5, shape, g, 1, idx_a, ls_indb, idx_b)))
        q = f["sns_vq"] if st == 0 else None
        return st == 0 and (q["shape"], q["gind"], q["idx_a"], q["ls_indb"], q["idx_b"]) == (shape, g, idx_a, ls_indb, idx_b)

    def largest(ok, hi):
        lo = 0  # ok(lo) holds, ok(hi) does not
        assert ok(lo) and not ok(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        return lo

    top = {s: largest(lambda i, s=s: valid(s, i), 1 << 24) for s in range(4)}
    b = largest(lambda v: valid(0, top[0], v & 1, v >> 1), 1 << 6)
    return top, (b >> 1, b & 1)


def _argtypes():
    f = O.lib().lc3o_kat_bitstream
    v, i = ctypes.c_void_p, ctypes.c_int
    f.argtypes = [i] * 8 + [v, v] + [i] * 4 + [v, i, i, i, v, v, i, v, i]
    f.restype = None


_argtypes()
