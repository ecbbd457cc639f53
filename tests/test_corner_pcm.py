"""Encoder corner PCM (corner_pcm.py: harmonic tones at 58 .. 100 Hz, full-scale DC / square / alternating samples, tones within 5 % of the
Nyquist frequency) at 20, 80 and 400 bytes in all 12 configurations (8 kHz under LC3GPU_SPEC_8KHZ_ENCODE): the device headers under the CPU
wave emulator byte-exact against the oracle encoder, the decoded PCM identical, and the census cells these signals are there for."""
import numpy as np
import pytest

import census_lib as N
import corner_pcm as P
import emu_lib
import inspect_lib as I
import oracle_lib as O

T = 8
SIZES = (20, 80, 400)


def oracle_bytes(kind, fs, us, nbytes):
    pcm = P.make(kind, T, I.config(fs, us).nf, fs)
    return pcm, O.encode_batch(pcm, nbytes, fs, us, spec_flags=1 if fs == 8000 else 0)


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_emulator_encodes_and_decodes_corner_pcm_as_the_oracle(fs, us, kind):
    nf = I.config(fs, us).nf
    for nbytes in SIZES:
        pcm, ref = oracle_bytes(kind, fs, us, nbytes)
        got = emu_lib.encode(pcm, nbytes, fs, us, spec_flags=1 if fs == 8000 else 0)
        bad = np.argwhere((got != ref).any(2))
        assert len(bad) == 0, "%s at %d Hz / %d us / %d bytes: frames (stream, frame) differing from the oracle encoder: %s" % (kind, fs, us, nbytes, bad[:8].tolist())
        assert np.array_equal(emu_lib.decode(ref, nf, fs, us), O.decode_batch(ref, nf, fs, us)), "%s at %d Hz / %d us / %d bytes: decoded PCM" % (kind, fs, us, nbytes)


@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_corner_pcm_reaches_its_cells(fs, us):
    """from the oracle alone: the long lags, present and active, at 20 bytes; escape depth 13 at 400 bytes; the global gain index raised to
    gg_min; the near-Nyquist flag at the rates whose coded band reaches the Nyquist frequency (at 44.1 and 48 kHz the 400 / 300 coded lines
    end at 20 kHz, below every tone within 5 % of fs / 2: no signal sets the flag there)"""
    def run(kind, nbytes):
        O.encoder_corner_counts(reset=True)
        _, data = oracle_bytes(kind, fs, us, nbytes)
        near_nyquist, gg_min = O.encoder_corner_counts(reset=True)
        return N.census(fs, us, [list(s) for s in data]), near_nyquist, gg_min

    cen, _, _ = run("harmonic_low", 20)
    assert cen["pitch=high/active"] >= N.FLOOR, cen["pitch=high/active"]
    cen, _, gg_min = run("full_scale", 400)
    assert cen["escape=13"] >= N.FLOOR and gg_min >= N.FLOOR, (cen["escape=13"], gg_min)
    if fs <= 32000:
        for kind in ("near_nyquist", "full_scale"):  # the alternating samples are a tone AT fs / 2
            assert run(kind, 20)[1] >= N.FLOOR, kind
