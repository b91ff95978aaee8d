"""`merfin -merge` end to end: two read files counted on their own and merged are byte for byte the database of both counted together --
the property users rely on -- with and without -passes; `-merge whole -min 2` is the database without its singletons; the stderr line's
numbers; no spool `<output>.blocks` stays."""
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import synth_reads as sr
from tests.test_cli import run
from tests.test_gpu_cli_count import _write_fastq

pytestmark = pytest.mark.gpu

MERGED = re.compile(r"-- Merged: (\d+) k-mers read, (\d+) written, (\d+) filtered, (\d+) saturated, (\d+) windows?\.\n")


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _count(tmp_path, name, k, files, extra=()):
    out = str(tmp_path / name)
    args = ["-count", "-k", str(k), "-output", out] + list(extra)
    for f in files:
        args += ["-reads", f]
    env = dict(os.environ, MFX_COUNT_BATCH="4096")
    env.pop("MFX_COUNT_WRITER", None)
    r = run(args, env=env)
    assert r.returncode == 0, r.stderr
    return out


def _merge(tmp_path, name, inputs, extra=(), **env):
    out = str(tmp_path / name)
    args = ["-output", out] + list(extra)
    for f in inputs:
        args += ["-merge", f]
    e = dict(os.environ)
    e.pop("MFX_MERGE_RANGE", None)
    e.update(env)
    r = run(args, env=e)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(out + ".blocks")
    got = MERGED.search(r.stderr)
    assert got and r.stderr.endswith("Bye!\n"), r.stderr
    return out, [int(x) for x in got.groups()], r.stderr


@pytest.mark.parametrize("k", [21, 31])
def test_counted_apart_and_merged_is_counted_together(tmp_path, k):
    m = _mfx()
    _, reads = sr.reads_world(k, 2600 + k, sizes=(12000, 4096, 500), n_reads=800)
    reads = [x for x in reads if x]
    half = len(reads) // 2
    fa, fb = str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq")
    _write_fastq(fa, reads[:half])
    _write_fastq(fb, reads[half:])
    whole = _count(tmp_path, "whole.mfxk", k, [fa, fb])
    rk, rv = po.count_kmers(k, reads)
    assert len(rk) > 3 * 4096
    want = str(tmp_path / "want.mfxk")
    m.db_write_flat(want, k, rk, rv)
    assert _bytes(whole) == _bytes(want)
    a = _count(tmp_path, "a.mfxk", k, [fa])
    b = _count(tmp_path, "b.mfxk", k, [fb])
    b3 = _count(tmp_path, "b3.mfxk", k, [fb], ("-passes", "3"))
    na, nb = m.db_probe(a)["n_kmers"], m.db_probe(b)["n_kmers"]
    for tag, second, env in (("ab", b, {}), ("ab3", b3, {}), ("ab_windows", b, {"MFX_MERGE_RANGE": "3000", "MFX_DB_BOUNCE": "4096"})):
        out, (n_read, n_written, n_filtered, n_saturated, windows), err = _merge(tmp_path, tag + ".mfxk", [a, second], **env)
        assert _bytes(out) == _bytes(whole), tag
        assert (n_read, n_written, n_filtered, n_saturated) == (na + nb, len(rk), 0, 0)
        assert (windows == 1) == (not env)
        assert "-- Wrote %d k-mers in " % len(rk) in err
    # -merge whole -min 2: the singletons gone
    keep = rv >= 2
    m.db_write_flat(want, k, rk[keep], rv[keep])
    out, nums, err = _merge(tmp_path, "min2.mfxk", [whole], ("-min", "2"))
    assert _bytes(out) == _bytes(want)
    assert nums[:4] == [len(rk), int(keep.sum()), int((~keep).sum()), 0]
    # the other operations, against the oracle's counts of the two halves
    ka, va = po.count_kmers(k, reads[:half])
    kb, vb = po.count_kmers(k, reads[half:])
    both = np.intersect1d(ka, kb)
    lo = np.minimum(va[np.searchsorted(ka, both)], vb[np.searchsorted(kb, both)])
    m.db_write_flat(want, k, both, lo)
    out, nums, err = _merge(tmp_path, "both.mfxk", [a, b], ("-op", "intersect"))
    assert _bytes(out) == _bytes(want) and nums[:4] == [na + nb, len(both), 0, 0]
    # MFX_DB_TIMING: the merge's split
    out, nums, err = _merge(tmp_path, "timed.mfxk", [a, b], MFX_DB_TIMING="1")
    assert "[mfx db] merge: read " in err and " decode " in err and " merge " in err and " combine " in err and "spool write " in err, err


def test_refused_merge_leaves_nothing(tmp_path):
    m = _mfx()
    k = 15
    keys = np.arange(0, 9000, 3, dtype=np.uint64)
    a = str(tmp_path / "a.mfxk")
    m.db_write_flat(a, k, keys, np.ones(len(keys), dtype=np.uint32))
    before = _bytes(a)
    out = str(tmp_path / "none" / "x.mfxk")                        # an output whose directory does not exist: the spool cannot be created
    r = run(["-merge", a, "-output", out])
    assert r.returncode == 1 and "cannot create the spool" in r.stderr, r.stderr
    text = tmp_path / "print.txt"
    text.write_text("AAAAAAAAAAAAAAC\t3\n")
    out = str(tmp_path / "y.mfxk")
    r = run(["-merge", a, "-merge", str(text), "-output", out])
    assert r.returncode == 1 and "run `merfin -convert` first" in r.stderr and "print.txt" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".blocks") and _bytes(a) == before
