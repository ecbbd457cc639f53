"""The composed corpus: per configuration some eighty streams of ten frames whose contents are chosen field by field (compose_lib), so that
the decoder and lc3gpu_inspect meet the parts of the LC3 format that the project's own encoder never writes -- the middle range of the
pitch index, an active post-filter at every gain step, the lower bandwidth indices at the high rates, every TNS order and both ends of
its coefficient range, every first-stage SNS index, all escape depths, lsb mode at any size, saturating output, and the frames a parser
must reject.  Generated from fixed seeds through the oracle; census_lib.cells() names what it has to hold.  Test infrastructure only.

A stream is (name, frames): ten frames of ONE size, so that streams of equal size go through the uniform calls together.  The frames of the
long-term post-filter streams carry real spectra (a harmonic tone through the oracle encoder, rewritten with chosen pitch fields): the
filter needs periodic content to act on.  Everything else carries small random integers.

Two cells one might look for do not exist.  No escape depth is rejected: the oracle's parser (as the reference's) leaves its escape loop
after 14 levels and goes on, and the writer's 16-bit lines end at depth 13, which it accepts.  And no frame takes the oracle's float chain
out of the finite range: global gain index 255 over lines of 32 767 through two order-8 TNS filters at the largest coefficient and the
largest SNS gains reaches some 4e16 (lc3o_kat_decode_stages), far beyond int32 -- the stream output/beyond-int32, where the conversion
to PCM itself has to saturate -- and far below 3.4e38."""
import functools

import numpy as np

import census_lib as N
import compose_lib as C
import inspect_lib as I
import oracle_lib as O

T = 10
BASE_10, BASE_75 = (40, 50, 60, 80, 100), (30, 38, 45, 60, 75)  # a size per fs_ind at which an active post-filter has a non-zero gain


def base_size(fs, us):
    return (BASE_10 if us == 10000 else BASE_75)[C.fs_index(fs)]


def tone_frames(fs, us, nbytes, n, seed):
    """n frames of a harmonic tone (a fundamental between 150 and 320 Hz with slow vibrato and its overtones, below 3.4 kHz under an even
    seed and up to 0.42 fs under an odd one) from the oracle encoder, after two frames of run-in"""
    cfg = I.config(fs, us)
    rng = np.random.default_rng([fs, us, seed])
    t = np.arange((n + 2) * cfg.nf) / float(fs)
    f0 = rng.uniform(150.0, 320.0)
    phase = 2 * np.pi * f0 * t + 1.5 * np.sin(2 * np.pi * rng.uniform(1.0, 3.0) * t)
    sig = sum(rng.uniform(0.3, 1.0) / h * np.sin(h * phase + rng.uniform(0, 6.28)) for h in range(1, int(min(3400.0 if seed % 2 == 0 else 1e9, 0.42 * fs) / f0) + 1))
    pcm = np.round(6000.0 * sig / np.abs(sig).max()).astype(np.int16).reshape(1, n + 2, cfg.nf)
    return O.encode_batch(pcm, nbytes, fs, us, spec_flags=1 if fs == 8000 else 0)[0][2:]


def _spectrum(rng, ne, n_lines, hi=3, upto=None):
    """n_lines non-zero lines of magnitude 1 .. hi at random places below `upto`"""
    x = np.zeros(ne, np.int64)
    at = rng.choice(upto or ne, min(n_lines, upto or ne), replace=False)
    x[at] = rng.integers(1, hi + 1, len(at)) * rng.choice([-1, 1], len(at))
    return x


class _Builder:
    def __init__(self, fs, us):
        self.fs, self.us = fs, us
        self.cfg = I.config(fs, us)
        self.ne, self.fi = self.cfg.ne, self.cfg.fs_ind
        self.base = base_size(fs, us)
        self.rng = np.random.default_rng([fs, us, 2])
        self.streams = []
        self.ins = I.OracleInspector(fs, us)

    def frame(self, nbytes, reject=False, **fields):
        """compose, and hold the frame to the oracle's parser: status 0, or non-zero for a reject cell.  A frame that does not fit its size
        is not the cell's frame: the caller asks for a larger size"""
        fr = C.compose(self.fs, self.us, nbytes, **fields)
        st = int(self.ins.record(fr)[0])
        assert (st != 0) == reject, "%d Hz / %d us, %d bytes: parser status %d for %s" % (self.fs, self.us, nbytes, st, sorted(fields))
        return fr

    def stream(self, name, size, specs):
        """ten frames from their field lists at `size`, or at the next larger size (in steps of 8 bytes) at which every one of them fits: a
        cell that cannot be composed at a small size is composed at a larger one, not dropped.  Not for the cells that hang on the size"""
        while True:
            try:
                self.add(name, [self.frame(size, **f) for f in specs])
                return
            except AssertionError:
                if size + 8 > 400:
                    raise
                size += 8

    def add(self, name, frames):
        assert len(frames) == T and len({len(f) for f in frames}) == 1, name
        self.streams.append((name, [np.asarray(f, np.uint8) for f in frames]))

    # ---------------------------------------------------------------- long-term post-filter
    def ltpf_stream(self, name, plan, nbytes, seed):
        """plan: per frame None (no pitch), ("A", index) active or ("I", index) present but inactive"""
        src = tone_frames(self.fs, self.us, min(self.base, nbytes) - 3, T, seed)  # three bytes of slack for the pitch fields
        out = []
        for fr, p in zip(src, plan):
            ch = dict(pitch_present=0, ltpf_active=0, pitch_index=0) if p is None else dict(pitch_present=1, ltpf_active=int(p[0] == "A"), pitch_index=p[1])
            out.append(C.rewrite(self.fs, self.us, fr, nbytes=nbytes, **ch))
        self.add(name, out)

    def pitch(self):
        A, In = (lambda v: ("A", v)), (lambda v: ("I", v))
        up = [0, 0, 379, 380, 381, 381, 438, 439, 440, 511]
        hop = [511, 0, 440, 379, 439, 380, 438, 381, 0, 511]
        for k, seq in enumerate((up, up[::-1], hop, hop[::-1])):
            self.ltpf_stream("pitch/ranges-%d" % k, [A(v) for v in seq], self.base, k)
        self.ltpf_stream("pitch/inactive-between-0", [A(0), In(380), A(379), In(0), A(380), In(511), A(439), None, A(440), A(511)], self.base, 4)
        self.ltpf_stream("pitch/inactive-between-1", [A(511), In(100), A(381), In(439), A(438), None, A(0), In(440), None, A(381)], self.base, 5)
        self.ltpf_stream("pitch/inactive-between-2", [In(379), A(440), In(381), None, A(379), In(450), In(300), A(438), In(480), In(400)], self.base, 6)
        # every transition with every pitch_frac the rate has: lags of one frac from the three ranges, twice
        by_frac = {}
        for p in list(range(380, 440)) + list(range(440, 512)) + list(range(380)):
            by_frac.setdefault(N.pitch_lag(self.fs, p)[1], []).append(p)
        for f, ps in sorted(by_frac.items()):
            lags = []
            for p in ps:  # three indices of this frac with different lags
                if N.pitch_lag(self.fs, p) not in [N.pitch_lag(self.fs, q) for q in lags]:
                    lags.append(p)
            for rep in range(2):
                a, b, c = (lags[(3 * rep + i) % len(lags)] for i in range(3))
                assert len({N.pitch_lag(self.fs, v) for v in (a, b, c)}) == 3
                self.ltpf_stream("pitch/frac-%d-%d" % (f, rep), [A(a), A(a), In(b), A(b), A(b), A(c), None, A(c), A(a), A(b)], self.base, 10 + 2 * f + rep)

    def filter_gain(self):
        sizes = sorted({n for _, below, at in N.gain_edge_sizes(self.fs, self.us) for n in (below, at)}) + [200]
        for k, n in enumerate(sizes):
            a, b = 100 + 37 * k, 390 + 5 * k
            plan = [("A", a), ("A", a), ("I", b), ("A", b), ("A", 445 + k), ("A", 445 + k), None, ("A", a), ("A", b), ("A", b)]
            self.ltpf_stream("ltpf-gain/%d-bytes" % n, plan, n, 30 + k)

    # ---------------------------------------------------------------- bandwidth, TNS
    def tns_fields(self, orders, rc=None):
        rc = self.rng.integers(3, 14, 16) if rc is None else rc
        return dict(tns_orders=orders, rc_i=[int(v) for v in rc])

    def bandwidth(self):
        stop = (80, 160, 240, 320, 400) if self.us == 10000 else (60, 120, 180, 240, 300)
        for bw in range(self.fi + 1):  # each with both TNS filters running and noise filling on
            specs = [dict(x_q=_spectrum(self.rng, self.ne, 6 + t, upto=min(stop[bw], self.ne)), bw=bw, noise_factor=(t + 1) % 8, gg_ind=150 + 3 * t,
                          **self.tns_fields((1 + (t + bw) % 8, 1 + (3 * t) % 8))) for t in range(T)]
            self.stream("bandwidth/%d" % bw, self.base, specs)
        if "status=%d" % (I.SIDE_INFO + 2) in N.cells(self.fs, self.us):
            specs = [dict(reject=t in (1, 4, 5, 7, 9), x_q=_spectrum(self.rng, self.ne, 8), bw=self.fi + (t in (1, 4, 5, 7, 9)), noise_factor=2, gg_ind=160)
                     for t in range(T)]
            self.stream("bandwidth/max+1", self.base, specs)

    def tns(self):
        nfilt = 2 if self.fi >= 3 else 1
        for size in N.weighting_sizes(self.us):
            for s in range(4):  # orders 1 .. 8 in each filter position, four frames each (the second filter's run against the first's)
                specs = [dict(x_q=_spectrum(self.rng, self.ne, 6), gg_ind=150, noise_factor=4,
                              **self.tns_fields(((s * T + t) % 8 + 1, 8 - (s * T + t) % 8 if nfilt == 2 else 0))) for t in range(T)]
                self.add("tns/orders-%d-bytes-%d" % (size, s), [self.frame(size, **f) for f in specs])
        pats = [[0, 16] * 8, [16, 0] * 8, [0] * 16, [16] * 16, [0, 0, 16, 16] * 4]
        for s in range(2):
            specs = []
            for t in range(T):
                rc = np.array(pats[t % 5])
                if t >= 5:  # the extreme value at some places only, ordinary values between them
                    rc = np.where(self.rng.random(16) < 0.5, rc, self.rng.integers(5, 12, 16))
                    rc[t - 5 + 8 * s::5] = pats[t % 5][0]
                specs.append(dict(x_q=_spectrum(self.rng, self.ne, 12), gg_ind=140, **self.tns_fields((8, 8 if nfilt == 2 else 0), rc)))
            self.stream("tns/rc-ends-%d" % s, self.base, specs)
        specs = [dict(x_q=_spectrum(self.rng, self.ne, 3, upto=2 + 2 * (t % 4)), lastnz=2 + 2 * (t % 4), gg_ind=170,
                      **self.tns_fields((1 + t % 8, 8 - t % 8 if nfilt == 2 else 0))) for t in range(T)]
        self.stream("tns/lastnz-below-the-filter", self.base, specs)

    # ---------------------------------------------------------------- spectrum
    def spectrum(self):
        ne = self.ne
        for size in N.rate_flag_sizes(self.fs):
            for s in range(2):
                fr = []
                for t in range(T):
                    lastnz = (2, ne // 2, ne // 2 + 2, ne)[(t + s) % 4]
                    x = _spectrum(self.rng, ne, 3, hi=2, upto=lastnz)
                    x[lastnz - 1 - (t & 1)] = 1 + t % 2
                    fr.append(self.frame(size, x_q=x, lastnz=lastnz, gg_ind=150, noise_factor=3))
                self.add("spectrum/lastnz-%d-bytes-%d" % (size, s), fr)
        for s in range(6):  # a pair of depth 13 takes some ninety bits
            specs = []
            for t in range(T):
                d = (s * T + t) % 14
                x = _spectrum(self.rng, ne, 4, upto=ne // 2)
                k = 2 * int(self.rng.integers(0, ne // 2))
                lo, hi = (0, 3) if d == 0 else (1 << (d + 1), (1 << (d + 2)) - 1)
                x[k], x[k + 1] = int(self.rng.integers(lo, hi + 1)) * (-1) ** t, int(self.rng.integers(0, hi + 1))
                specs.append(dict(x_q=x, gg_ind=60 + 5 * (t % 3), noise_factor=7))
            self.stream("spectrum/escape-%d" % s, max(self.base, 50), specs)

    def lsb_mode(self):
        ne = self.ne
        for size in (20, max(self.base, 60), 400):
            # a spectrum of few lines cannot use up a large frame even at the deepest escapes: the largest size at which the cell exists
            size = next(n for n in (size, 300, 200, 150, 120, 100, 80) if n <= size and self.lsb_frame(n, 0) is not None)
            self.add("lsb/mode-1-%d-bytes" % size, [self.lsb_frame(size, t) for t in range(T)])
        # lsb_mode = 0: fewer, exactly as many and more residual bits handed to the writer than the frame has room for
        for extra in (-3, 0, 5):
            fr = []
            for t in range(T):
                for n_lines in range(ne - 2, 3, -2):
                    x = _spectrum(self.rng, ne, n_lines, hi=2)
                    st, f = C.parse_full(self.fs, self.us, C.compose(self.fs, self.us, self.base, x_q=x, gg_ind=150, res_bits=[1] * 400))
                    if st == 0 and 6 <= len(f["res_bits"]) < n_lines:  # the budget ends before the lines do: it is the room
                        break
                else:
                    raise AssertionError("no spectrum leaves a residual budget shorter than its lines")
                bits = [1, 1, 1] + [int(b) for b in self.rng.integers(0, 2, len(f["res_bits"]) - 3 + extra)]
                fr.append(self.frame(self.base, x_q=x, gg_ind=150, res_bits=bits))
            self.add("lsb/mode-0-residual-%+d" % extra, fr)
        fr = [self.frame(200, x_q=_spectrum(self.rng, ne, 3 + t), gg_ind=150, res_bits=[t & 1] * 20) for t in range(T)]
        self.add("lsb/mode-0-room-for-all", fr)

    def lsb_frame(self, size, t):
        """lsb_mode = 1, every coded magnitude odd and at least 9 (one lsb bit per value, no sign among the lsb bits), more lsb bits than
        the frame has room for and the room an odd number: the walk ends between the two values of a pair.  None: no such frame"""
        ne = self.ne
        rng = np.random.default_rng([self.fs, self.us, size, t])
        for depth in range(2, 14):
            lo, hi = max(1 << (depth + 1), 9), (1 << (depth + 2)) - 1
            for n_pairs in range(ne // 2, 1, -1):
                x = np.zeros(ne, np.int64)
                x[:2 * n_pairs] = (rng.integers(lo // 2, hi // 2 + 1, 2 * n_pairs) * 2 + 1) * rng.choice([-1, 1], 2 * n_pairs)
                fr = C.compose(self.fs, self.us, size, x_q=x, lsb_mode=1, gg_ind=90 + t, noise_factor=5)
                tags, rec, got = N.frame_tags(self.fs, self.us, fr, self.ins)
                if rec[0]:
                    continue  # does not fit: fewer pairs
                if "lsb_cut_mid_pair" in tags:
                    return fr
                if (got[:2 * n_pairs] & 1).all():
                    break  # room for every lsb bit, and fewer pairs leave more: a deeper spectrum
        return None

    # ---------------------------------------------------------------- noise, SNS, gain
    def noise(self):
        for kind in ("zero", "sparse"):
            for s in range(4):
                specs = []
                for t in range(T):
                    x = np.zeros(self.ne, np.int64) if kind == "zero" else _spectrum(self.rng, self.ne, 2 + t % 5)
                    gg = 0 if kind == "zero" and (t + s) % 5 == 0 else 150 + 4 * t  # index 0 on an all-zero frame: the zero-frame flag
                    specs.append(dict(x_q=x, noise_factor=(t + 3 * s) % 8, gg_ind=gg))
                self.stream("noise/%s-%d" % (kind, s), self.base, specs)

    def sns(self):
        top, (b_max, ls_max) = C.sns_index_limits()
        for s in range(13):
            specs = []
            for t in range(T):
                i = s * T + t
                shape = i % 4
                g = (0, C.SNS_GAINS[shape] - 1, int(self.rng.integers(0, C.SNS_GAINS[shape])))[(i // 4) % 3]
                idx_a = (0, top[shape], int(self.rng.integers(0, top[shape] + 1)))[(i // 12 + i // 4) % 3]
                idx_b, ls_b = ((0, 0), (b_max, ls_max), (int(self.rng.integers(0, b_max + 1)), int(self.rng.integers(0, 2))))[(i // 8) % 3]
                q = C.sns(i % 32, (7 * i + 3) % 32, shape, g, i & 1, idx_a, ls_b if shape == 0 else 0, idx_b if shape == 0 else 0)
                specs.append(dict(x_q=_spectrum(self.rng, self.ne, 12), sns_vq=q, gg_ind=150, noise_factor=2))
            self.stream("sns/%d" % s, self.base, specs)
        for s in range(2):
            specs = []
            for t in range(T):
                kind = (0, 1, 0, 2, 0, 0, 1, 2, 1, 2)[(t + s) % T]  # 1: the first invalid index of the 25-bit field, 2: of the 24-bit field
                q = (C.sns(1, 2, 2, 1, 0, 12345), C.sns(4, 9, 0, 1, 1, top[0] + 1, ls_max, b_max), C.sns(30, 31, 3, 7, 0, top[3] + 1))[kind]
                specs.append(dict(reject=kind != 0, x_q=_spectrum(self.rng, self.ne, 9), sns_vq=q, gg_ind=155, noise_factor=1))
            self.stream("sns/first-invalid-index-%d" % s, self.base, specs)

    def gain_and_output(self):
        specs = [dict(x_q=_spectrum(self.rng, self.ne, 10, hi=12), gg_ind=0 if t % 2 else 255, noise_factor=t % 8) for t in range(T)]
        self.stream("output/gain-0-and-255", self.base, specs)
        specs = []
        for t in range(T):  # index 255 (and 236) over lines of up to 29 000: the PCM is clipped at both ends within the frame
            x = _spectrum(self.rng, self.ne, 6, hi=3)
            x[self.rng.choice(self.ne // 2, 3, replace=False)] = [20000 + 1000 * t, -(9000 + t), 3000]
            specs.append(dict(x_q=x, gg_ind=255 if t % 3 else 236, noise_factor=0))
        self.stream("output/saturating", max(self.base, 60), specs)
        specs = []
        for t in range(T):  # the float chain at its largest (some 1e16, far beyond int32: the conversion itself has to saturate); it stays finite
            x = np.zeros(self.ne, np.int64)
            x[12:20] = self.rng.integers(30000, 32768, 8) * self.rng.choice([-1, 1], 8)
            specs.append(dict(x_q=x, gg_ind=255, sns_vq=C.sns(t, 31 - t, 3, 7), **self.tns_fields((8, 8), [16] * 16 if t % 2 else [16, 0] * 8)))
        self.stream("output/beyond-int32", 100, specs)

    def build(self):
        for topic in (self.pitch, self.filter_gain, self.bandwidth, self.tns, self.spectrum, self.lsb_mode, self.noise, self.sns, self.gain_and_output):
            topic()
        return self.streams


@functools.lru_cache(None)
def corpus(fs, us):
    """[(name, [frame] * T)]; built once per configuration and shared by the tests, which leave it unchanged"""
    return tuple(_Builder(fs, us).build())


SIZED_TOPICS = ("ltpf-gain/", "spectrum/lastnz", "tns/orders", "lsb/")  # the cells whose frames differ with the frame size


def by_size(fs, us):
    """{nbytes: (names, uint8[S][T][nbytes])}"""
    groups = {}
    for name, frames in corpus(fs, us):
        groups.setdefault(len(frames[0]), []).append((name, np.stack(frames)))
    return {n: ([k for k, _ in v], np.stack([f for _, f in v])) for n, v in sorted(groups.items())}


def sized_streams(fs, us):
    """(names, data uint8[S][T][400], nb uint16[S][T]): the size-dependent streams cut along the diagonal, so that a stream's size changes
    from frame to frame; frame t of stream s is frame t of the corpus stream (s + t) mod S"""
    src = [(n, f) for n, f in corpus(fs, us) if n.startswith(SIZED_TOPICS)]
    S = len(src)
    src = [src[i] for i in np.random.default_rng(S).permutation(S)]  # neighbours in the corpus share their size
    data, nb = np.zeros((S, T, 400), np.uint8), np.zeros((S, T), np.uint16)
    for s in range(S):
        for t in range(T):
            fr = src[(s + t) % S][1][t]
            data[s, t, :len(fr)] = fr
            nb[s, t] = len(fr)
    return [n for n, _ in src], data, nb


@functools.lru_cache(None)
def oracle_pcm(fs, us):
    """{nbytes: int16[S][T][nf]} of by_size(fs, us), from the oracle decoder"""
    nf = I.config(fs, us).nf
    return {n: O.decode_batch(data, nf, fs, us) for n, (_, data) in by_size(fs, us).items()}


def oracle_pcm_sized(fs, us):
    nf = I.config(fs, us).nf
    _, data, nb = sized_streams(fs, us)
    out = np.zeros(nb.shape + (nf,), np.int16)
    for s in range(len(data)):
        dec = O.Decoder(fs, us)
        for t in range(T):
            out[s, t] = dec.decode_frame(data[s, t, :nb[s, t]])[1]
    return out
