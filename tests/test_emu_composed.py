"""The composed corpus (composed_corpus.py: frames with chosen contents in the corners of the format that the project's own encoder never
reaches) through the device headers under the CPU wave emulator, at all 12 configurations: the decoder with the reconstruction on the
parser's lane and in its late form against the oracle's PCM, and the frame inspection against the oracle's records, the frames a parser
must reject included.  Identical 16-bit PCM and identical records: no tolerance."""
import numpy as np
import pytest

import composed_corpus as CC
import emu_lib
import inspect_lib as I
import test_emu_inspect as EI

emu = EI.emu  # the inspection emulator, built once per module


@pytest.mark.parametrize("late", [0, 1])
@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_decode_composed_against_the_oracle(fs, us, late):
    nf = I.config(fs, us).nf
    ref = CC.oracle_pcm(fs, us)
    for nbytes, (names, data) in CC.by_size(fs, us).items():
        got = emu_lib.decode(data, nf, fs, us, late=late)
        bad = np.argwhere((got != ref[nbytes]).any(2))
        assert len(bad) == 0, "%d Hz / %d us, %d bytes, late=%d: %d frames differ from the oracle; first: stream %s frame %d, largest difference %d" % (
            fs, us, nbytes, late, len(bad), names[bad[0][0]], bad[0][1], np.abs(got.astype(int) - ref[nbytes]).max())


@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_inspect_composed_against_the_oracle(emu, fs, us):
    frames = [f for _, fr in CC.corpus(fs, us) for f in fr]
    data = np.zeros((len(frames), 400), np.uint8)
    for i, f in enumerate(frames):
        data[i, :len(f)] = f
    nb = np.array([len(f) for f in frames], np.uint16)
    ref = EI._check(emu, fs, us, data, nb)
    assert (ref[:, 0] != 0).sum() >= 8, "the reject cells"
