"""The coefficient tables of lc3gpu_resample_mixed_views (tables/lc3_resample_tables.h, written by tools/gen_resample_tables.py): the
committed header against the formula of include/lc3gpu.h recomputed here in float64, the two sums every phase must have (exactly 32768, and
sum |c| <= 65535: what keeps the device's int32 accumulator exact), the frequency response of the twelve quantised prototypes inside two
design bounds, and the numpy model (resample_lib) on a constant and on a sine.  No GPU needed."""
import math
import os
import subprocess
import sys

import numpy as np

import resample_lib as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _formula(L, M):
    """the header comment's recipe, written out once more (not the generator's code)"""
    Q = max(L, M)
    N = 16 * Q + 1
    fc = 0.92 * 0.5 / Q
    h = np.array([L * 2 * fc * np.sinc(2 * fc * (n - 8 * Q)) for n in range(N)], np.float64) * np.kaiser(N, 6.0)
    T = -(-N // L)
    out = np.zeros((L, T), np.int64)
    for p in range(L):
        taps = np.array([h[p + L * j] if p + L * j < N else 0.0 for j in range(T)])
        scaled = taps / taps.sum() * 32768.0
        q = np.rint(scaled).astype(np.int64)
        q[np.argmax(np.abs(scaled))] += 32768 - q.sum()
        out[p] = q
    return out


def test_the_twelve_ratios_are_the_ones_of_the_twenty_pairs():
    tabs = R.tables()
    assert len(R.PAIRS) == 20 and len(tabs) == 12
    assert set(tabs) == {R.ratio_of(fi, fo) for fi, fo in R.PAIRS}
    assert all(1 <= L <= 6 and 1 <= M <= 6 and math.gcd(L, M) == 1 for L, M in tabs)
    for (L, M), c in tabs.items():
        assert c.shape == (L, -(-(16 * max(L, M) + 1) // L))
        assert c.shape[1] == 17 or L < M  # every up-ratio has 17 taps per phase
    assert max(c.shape[1] for c in tabs.values()) == 97 == tabs[(1, 6)].shape[1]
    # S_out * M == S_in * L for every pair and both durations, and a chunk of the plan starts at phase 0
    for fi, fo in R.PAIRS:
        L, M = R.ratio_of(fi, fo)
        for us in (7500, 10000):
            assert R.nf_of(fo, us) * M == R.nf_of(fi, us) * L


def test_the_committed_header_is_the_formula_in_float64():
    for (L, M), c in R.tables().items():
        assert np.array_equal(c, _formula(L, M)), (L, M)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_resample_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_every_phase_sums_to_32768_and_the_accumulator_bound_holds():
    worst_c, worst_sum = 0, 0
    for (L, M), c in R.tables().items():
        assert (c.sum(axis=1) == 32768).all(), (L, M)
        assert np.abs(c).max() <= 32767, (L, M)
        assert (np.abs(c).sum(axis=1) <= 65535).all(), (L, M)
        worst_c, worst_sum = max(worst_c, int(np.abs(c).max())), max(worst_sum, int(np.abs(c).sum(axis=1).max()))
    print("max |c| %d, max sum |c| %d" % (worst_c, worst_sum))
    assert (worst_c, worst_sum) == (30144, 60988)  # (the figures the header comment states)
    assert 32768 * 65535 + 16384 < 2**31


def test_the_frequency_response_of_every_quantised_prototype_stays_inside_the_design_bounds():
    """passband ripple <= 0.1 dB up to 0.7 of the lower Nyquist, stopband <= -60 dB from 1.3 of it, on the int16 table itself (measured:
    0.039 dB and -65.2 dB at worst)"""
    f = np.linspace(0.0, 0.5, 8001)
    worst = [0.0, -999.0]
    for (L, M), c in R.tables().items():
        h = np.zeros(c.size)
        for p in range(L):
            h[p::L] = c[p] / 32768.0
        H = np.abs(np.exp(-2j * np.pi * f[:, None] * np.arange(len(h))[None, :]) @ h) / L
        nyq = 0.5 / max(L, M)
        ripple = float(np.abs(20 * np.log10(H[f <= 0.7 * nyq])).max())
        stop = float(20 * np.log10(H[f >= 1.3 * nyq].max()))
        print("L %d M %d: ripple %.4f dB, stopband %.2f dB" % (L, M, ripple, stop))
        assert ripple <= 0.1 and stop <= -60.0, (L, M, ripple, stop)
        worst = [max(worst[0], ripple), max(worst[1], stop)]
    print("worst: ripple %.4f dB, stopband %.2f dB" % tuple(worst))


def test_a_constant_input_gives_exactly_that_constant_after_the_warm_up():
    for fi, fo in R.PAIRS + R.COPIES:
        T = R.taps_of(fi, fo)
        L, M = R.ratio_of(fi, fo)
        for v in (32767, -32768, 1, -1, 12345):
            out, hist = R.resample(np.full(fi // 100 * 2, v), np.zeros(T - 1), fi, fo)
            warm = -(-(T - 1) * L // M)  # the first output whose taps all lie at or behind x[0]
            assert (out[warm:] == v).all() and len(out) == fo // 100 * 2, (fi, fo, v)
            assert len(hist) == T - 1 and (hist == v).all()


def test_a_1_khz_sine_through_all_twenty_pairs_keeps_its_snr():
    """a 1 kHz sine of amplitude 20000 (rounded to int16), 0.4 s, through the model from a fresh history, against the sine delayed by the
    group delay (8 samples of the lower rate), from output sample 200 on.  SNR in dB, fs_in -> fs_out:
         8000 -> 16000  87.8     8000 -> 24000  79.8     8000 -> 32000  80.9     8000 -> 48000  80.8
        16000 ->  8000  73.9    16000 -> 24000  66.1    16000 -> 32000  69.8    16000 -> 48000  66.1
        24000 ->  8000 103.4    24000 -> 16000  65.1    24000 -> 32000  66.1    24000 -> 48000  71.8
        32000 ->  8000 103.4    32000 -> 16000  77.7    32000 -> 24000  65.7    32000 -> 48000  69.4
        48000 ->  8000  81.6    48000 -> 16000  67.7    48000 -> 24000  77.2    48000 -> 32000  70.8
    The model is deterministic; the floor is 3 dB below the worst of them (65.1) and only guards later edits of the table."""
    worst = 1e9
    for fi, fo in R.PAIRS:
        t = np.arange(fi // 10 * 4) / fi
        x = np.rint(20000 * np.sin(2 * np.pi * 1000 * t)).astype(np.int64)
        out, _ = R.resample(x, np.zeros(R.taps_of(fi, fo) - 1), fi, fo)
        m = np.arange(len(out))
        ideal = 20000 * np.sin(2 * np.pi * 1000 * (m / fo - 8 / min(fi, fo)))
        err = out[200:] - ideal[200:]
        snr = 10 * np.log10((ideal[200:] ** 2).sum() / (err ** 2).sum())
        print("%5d -> %5d %.1f dB" % (fi, fo, snr))
        worst = min(worst, snr)
    assert worst >= 62.1, worst
