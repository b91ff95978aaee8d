"""The device encoder of the streamed database writer (csrc/mfx_sort.hip: mfx_delta_plan_kernel, mfx_delta_pack_kernel with mfx_delta_word)
against the Python encoder's bytes, over the whole writers' catalogue (tests/encoder_blocks.py: every kbits 1 .. 62 and vbits 2 .. 22 in a
full block, the cost edges of the vbits rule, the escape positions at the wave and round seams -- asserted on the reference alone in
tests/test_encoder_blocks_cpu.py, where both host writers also give these bytes).  The expected file is delta_blocks.encode_counts', which
shares no code with the library.  Every route writes every world whole, byte for byte:
  table     Index.add_read / add_asm, then write_db(streamed=True): one append of all full blocks
  merge     db_merge of the Python encoder's own file, one window: the decode kernel reads every width in the same run, and the output
            is the input
  windows   the same under MFX_MERGE_RANGE=3000 (appends of at most one block behind a carry), and db_merge_except with an empty
            subtracted database
and the output loads back through Index.load_db / export.  A second run of each route gives the same bytes."""
import os

import numpy as np
import pytest

from tests import encoder_blocks as eb

pytestmark = pytest.mark.gpu


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _first_difference(got, want):
    """where two files part: for the assertion's message"""
    if len(got) != len(want):
        return "length %d, expected %d" % (len(got), len(want))
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    at = np.flatnonzero(a != b)
    return "%d bytes differ, the first at %d" % (len(at), int(at[0])) if len(at) else "equal"


def _same(path, want, what):
    got = _read(path)
    assert got == want, (what, _first_difference(got, want))
    assert not os.path.exists(path + ".blocks")


def _unset(monkeypatch, *names):
    for n in names:
        monkeypatch.delenv(n, raising=False)


@pytest.mark.parametrize("name", eb.names())
def test_table_written_streamed(tmp_path, monkeypatch, name):
    m = _mfx()
    _unset(monkeypatch, "MFX_WRITE_DB_RANGE", "MFX_DB_BOUNCE")
    w = eb.world(name)
    want = eb.expected_bytes(w)
    n = len(w.kmers)
    zeros = np.zeros(n, dtype=np.uint32)
    for side in (0, 1):
        ix = m.Index(w.k, n + 64)
        (ix.add_asm if side else ix.add_read)(w.kmers, w.counts)
        for run in (0, 1):                                         # a second run: the same bytes
            out = str(tmp_path / ("t%d%d.mfxk" % (side, run)))
            assert ix.write_db(out, side, streamed=True) == n
            _same(out, want, (name, "table", side, run))
        ek, er, ea = ix.export()                                   # the table is unchanged
        np.testing.assert_array_equal(ek, w.kmers)
        np.testing.assert_array_equal(ea if side else er, w.counts)
        np.testing.assert_array_equal(er if side else ea, zeros)
        ix.close()
    back = m.Index(w.k, n + 64)                                    # the round trip through the table's decode kernel
    back.load_db(str(tmp_path / "t00.mfxk"), 0)
    ek, er, ea = back.export()
    np.testing.assert_array_equal(ek, w.kmers)
    np.testing.assert_array_equal(er, w.counts)
    assert not ea.any()


@pytest.mark.parametrize("name", eb.names())
def test_merge_of_the_python_encoders_file(tmp_path, monkeypatch, name):
    m = _mfx()
    w = eb.world(name)
    want = eb.expected_bytes(w)
    n = len(w.kmers)
    src, none = str(tmp_path / "python.mfxk"), str(tmp_path / "none.mfxk")
    with open(src, "wb") as f:
        f.write(want)
    m.db_write_flat(none, w.k, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    nblocks = len(w.blocks)
    for rng in (None, "3000"):
        if rng is None:
            _unset(monkeypatch, "MFX_MERGE_RANGE", "MFX_DB_BOUNCE")
        else:
            monkeypatch.setenv("MFX_MERGE_RANGE", rng)
        for run in (0, 1):
            out = str(tmp_path / ("m%s%d.mfxk" % (rng or "whole", run)))
            st = m.db_merge([src], out)
            assert (st["n_in"], st["n_out"], st["n_filtered"], st["n_saturated"]) == (n, n, 0, 0), st
            assert st["windows"] == 1 if rng is None else 2 <= st["windows"] <= nblocks + 1, st
            _same(out, want, (name, "merge", rng, run))
        if rng:
            out = str(tmp_path / "except.mfxk")
            st = m.db_merge_except([src], [none], out)
            assert (st["n_in"], st["n_out"], st["n_subtracted"]) == (n, n, 0) and st["windows"] >= 2, st
            _same(out, want, (name, "except", rng))
    assert _read(src) == want
