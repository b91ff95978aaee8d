"""`merfin -count`, with and without -passes, through the streamed database writer: the output is byte for byte the one of the host writer
(MFX_COUNT_WRITER=host) and mfx_db_write_flat of the oracle's counts, and no spool `<output>.blocks` stays behind a run, refused or not."""
import os

import pytest

from oracle import pyoracle as po
from tests import synth_reads as sr
from tests.test_cli import run
from tests.test_gpu_cli_count import _write_fastq

pytestmark = pytest.mark.gpu


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _run(tmp_path, name, k, fq, extra=(), **env):
    out = str(tmp_path / name)
    e = dict(os.environ, MFX_COUNT_BATCH="4096")
    e.pop("MFX_COUNT_WRITER", None)
    e.update(env)
    return out, run(["-count", "-reads", fq, "-k", str(k), "-output", out] + list(extra), env=e)


@pytest.mark.parametrize("k", [21, 31])
def test_count_streams_the_database(tmp_path, k):
    m = _mfx()
    _, reads = sr.reads_world(k, 1800 + k, sizes=(12000, 4096, 500), n_reads=800)
    reads = [x for x in reads if x]
    rk, rv = po.count_kmers(k, reads)
    assert len(rk) > 3 * 4096                                      # several blocks and a partial one
    fq = str(tmp_path / "reads.fastq")
    _write_fastq(fq, reads)
    want = str(tmp_path / "want.mfxk")
    m.db_write_flat(want, k, rk, rv)
    with open(want, "rb") as f:
        want_bytes = f.read()
    wrote = "-- Wrote %d k-mers in " % len(rk)
    for extra in ((), ("-passes", "3")):
        tag = "p3" if extra else "one"
        for env in ({}, {"MFX_COUNT_WRITER": "stream"}, {"MFX_COUNT_WRITER": "host"}, {"MFX_WRITE_DB_RANGE": "1000", "MFX_DB_BOUNCE": "4096"}):
            out, r = _run(tmp_path, "%s_%s.mfxk" % (tag, "_".join(env.values()) or "default"), k, fq, extra, **env)
            assert r.returncode == 0, r.stderr
            with open(out, "rb") as f:
                assert f.read() == want_bytes, (extra, env)
            assert not os.path.exists(out + ".blocks")
            assert wrote in r.stderr and r.stderr.endswith("Bye!\n")
    # MFX_DB_TIMING: the streamed writer's split, on stderr, from the default run
    out, r = _run(tmp_path, "timed.mfxk", k, fq, (), MFX_DB_TIMING="1")
    assert r.returncode == 0 and "[mfx db] streamed writer: export " in r.stderr and "spool write " in r.stderr, r.stderr
    out, r = _run(tmp_path, "timed_host.mfxk", k, fq, (), MFX_DB_TIMING="1", MFX_COUNT_WRITER="host")
    assert r.returncode == 0 and "[mfx db] streamed writer" not in r.stderr and "[mfx db] delta writer: " in r.stderr, r.stderr


def test_refused_runs_leave_no_spool(tmp_path):
    _mfx()
    k = 21
    _, reads = sr.reads_world(k, 1821, sizes=(12000, 4096, 500), n_reads=800)
    fq = str(tmp_path / "reads.fastq")
    _write_fastq(fq, [x for x in reads if x])
    # a -memory below the smallest table: the pass cannot begin, after the writer was opened
    for extra in (("-passes", "3"), ("-passes", "auto"), ()):
        out, r = _run(tmp_path, "refused.mfxk", k, fq, list(extra) + ["-memory", "0.0001"])
        assert r.returncode == 1 and "k-mer table" in r.stderr, r.stderr
        assert not os.path.exists(out) and not os.path.exists(out + ".blocks"), os.listdir(str(tmp_path))
    for extra in (("-passes", "2"), ()):
        out, r = _run(tmp_path, "knob.mfxk", k, fq, extra, MFX_COUNT_WRITER="disk")
        assert r.returncode == 1 and "ERROR: -count: MFX_COUNT_WRITER is 'stream' or 'host', not 'disk'." in r.stderr, r.stderr
        assert not os.path.exists(out) and not os.path.exists(out + ".blocks")
    # an output whose directory does not exist: the spool cannot be created
    out, r = _run(tmp_path / "none", "x.mfxk", k, fq, ("-passes", "2"))
    assert r.returncode == 1 and "cannot create the spool" in r.stderr, r.stderr
