"""PCM at the corners the encoder's usual test material never reaches: harmonic tones with a fundamental of 58 .. 100 Hz (the long lags:
pitch index 440 and above), full-scale DC, square wave and sign-alternating samples (the deepest escape codes, the global gain pushed up to
its lower limit), and tones within 5 % of the Nyquist frequency (the near-Nyquist flag that switches TNS and the post-filter off).
Deterministic; test infrastructure only (synth.py's generators are the benchmark's and stay as they are)."""
import numpy as np

KINDS = ("harmonic_low", "full_scale", "near_nyquist")


def harmonic_low(n_frames, nf, fs_hz):
    """four streams: fundamentals of 58, 71, 86 and 100 Hz with overtones falling off as 1 / h up to 1.2 kHz"""
    t = np.arange(n_frames * nf) / float(fs_hz)
    out = []
    for f0 in (58.0, 71.0, 86.0, 100.0):
        sig = sum(np.sin(2 * np.pi * h * f0 * t + 0.7 * h) / h for h in range(1, int(1200 / f0) + 1))
        out.append(np.round(12000.0 * sig / np.abs(sig).max()))
    return np.array(out).astype(np.int16).reshape(4, n_frames, nf)


def full_scale(n_frames, nf, fs_hz):
    """four streams: DC at +32767, DC at -32768, a square wave of 48 samples' period between the two, samples alternating between them"""
    n = n_frames * nf
    k = np.arange(n)
    square = np.where((k // 24) % 2 == 0, 32767, -32768)
    alt = np.where(k % 2 == 0, 32767, -32768)
    return np.array([np.full(n, 32767), np.full(n, -32768), square, alt]).astype(np.int16).reshape(4, n_frames, nf)


def near_nyquist(n_frames, nf, fs_hz):
    """three streams: tones at 95.5 %, 98 % and 99.7 % of fs / 2"""
    t = np.arange(n_frames * nf) / float(fs_hz)
    return np.array([np.round(20000.0 * np.sin(2 * np.pi * r * fs_hz / 2 * t + 0.3)) for r in (0.955, 0.98, 0.997)]).astype(np.int16).reshape(3, n_frames, nf)


def make(kind, n_frames, nf, fs_hz):
    return {"harmonic_low": harmonic_low, "full_scale": full_scale, "near_nyquist": near_nyquist}[kind](n_frames, nf, fs_hz)
