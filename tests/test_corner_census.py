"""The census of frame-format corners (census_lib): the composed corpus holds every cell of census_lib.cells() at least FLOOR times in every
configuration in which the cell exists -- a condition on the corpus, so that no cell of the composed-parity tests (test_emu_composed.py,
test_gpu_composed.py) rests on one lucky frame or drops out unnoticed -- and the same census of the benchmark's headline material, printed
as the record of what the project's own encoder reaches."""
import importlib

import numpy as np
import pytest

import census_lib as N
import composed_corpus as CC
import inspect_lib as I
import oracle_lib as O

synth = importlib.import_module("lc3-codec_amd.synth")


@pytest.mark.parametrize("fs,us", I.CONFIGS)
def test_composed_corpus_fills_every_cell(fs, us):
    streams = CC.corpus(fs, us)
    assert all(len(frames) == CC.T for _, frames in streams) and len({name for name, _ in streams}) == len(streams)
    counts = N.census(fs, us, [frames for _, frames in streams])
    print("%d Hz / %d us: %d streams, %d frames\n%s" % (fs, us, len(streams), CC.T * len(streams), N.report(counts)))
    short = [(c, counts[c]) for c in N.cells(fs, us) if counts[c] < N.FLOOR]
    assert not short, "%d Hz / %d us: cells with fewer than %d frames: %s" % (fs, us, N.FLOOR, short)


def test_a_removed_stream_empties_its_cell():
    """the check above notices a stream that drops out: without the stream of bandwidth index max + 1 its cell falls below the floor"""
    streams = [frames for name, frames in CC.corpus(48000, 10000) if name != "bandwidth/max+1"]
    assert len(streams) == len(CC.corpus(48000, 10000)) - 1
    cell = "status=%d" % (I.SIDE_INFO + 2)
    assert cell in N.cells(48000, 10000) and N.census(48000, 10000, streams)[cell] < N.FLOOR


def test_headline_material_census_for_the_record():
    """what the benchmark's material reaches: make_pcm(256, 8, 480, 48000) through the oracle encoder at 150 bytes, 2048 frames.  Printed
    (pytest -s), nothing asserted about the counts: the cells it leaves empty are why the composed corpus exists."""
    pcm = synth.make_pcm(256, 8, 480, 48000)
    data = O.encode_batch(pcm, 150, threads=8)
    counts = N.census(48000, 10000, [list(s) for s in data])
    assert sum(v for k, v in counts.items() if k.startswith("status=")) == 2048
    empty = [c for c in N.cells(48000, 10000) if counts[c] == 0]
    print("headline material, 2048 frames at 48 kHz / 10 ms / 150 bytes\n%s\ncells of the composed corpus it never reaches (%d of %d): %s"
          % (N.report(counts), len(empty), len(N.cells(48000, 10000)), " ".join(empty)))
