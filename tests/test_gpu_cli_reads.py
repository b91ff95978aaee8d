"""`merfin -hist / -dump -reads a.fq.gz -reads b.fa -k 21`: the histogram file, the dump and the summary lines are byte-identical
to a run on `-readmers` holding the same reads' counts; an -index image is rebuilt once a read file changes."""
import gzip
import os

import pytest

from oracle import pyoracle as po
from tests import synth_reads as sr
from tests.test_cli import _write_fasta, _write_text_db, run

pytestmark = pytest.mark.gpu


def _files(tmp_path, k):
    asm, reads = sr.reads_world(k, 4321)
    reads = [x for x in reads if x]                               # (a FASTQ record needs a base)
    fa = str(tmp_path / "asm.fa")
    _write_fasta(fa, asm)
    half = len(reads) // 2
    fq = str(tmp_path / "a.fq.gz")
    with gzip.open(fq, "wt") as f:
        for i, x in enumerate(reads[:half]):
            f.write("@r%d\n%s\n+\n%s\n" % (i, x.decode(), "I" * len(x)))
    fb = str(tmp_path / "b.fa")
    with open(fb, "w") as f:
        for i, x in enumerate(reads[half:]):
            f.write(">s%d\n%s\n" % (i, x.decode()))
    db = str(tmp_path / "reads.txt")
    rk, rv = po.count_kmers(k, reads)
    _write_text_db(db, k, rk, rv)
    return fa, fq, fb, db


def _summary(stderr):
    return [l for l in stderr.splitlines() if not l.startswith("--")]


@pytest.mark.parametrize("mode,devices", [("-hist", None), ("-dump", None), ("-hist", "0,0")])
def test_cli_reads_equal_the_database_route(tmp_path, mode, devices):
    k = 21
    fa, fq, fb, db = _files(tmp_path, k)
    dev = ["-devices", devices] if devices else []
    a = run([mode, "-sequence", fa, "-reads", fq, "-reads", fb, "-k", str(k), "-peak", "10", "-output", str(tmp_path / "a.out")] + dev)
    b = run([mode, "-sequence", fa, "-readmers", db, "-peak", "10", "-output", str(tmp_path / "b.out")] + dev)
    assert a.returncode == 0, a.stderr
    assert b.returncode == 0, b.stderr
    assert open(tmp_path / "a.out", "rb").read() == open(tmp_path / "b.out", "rb").read()
    assert _summary(a.stderr) == _summary(b.stderr)
    line = [l for l in a.stderr.splitlines() if l.startswith("-- Counted the 21-mers of")]
    assert len(line) == 1 and " counted, " in line[0] and " dropped." in line[0]


def test_cli_reads_index_image_follows_the_read_files(tmp_path):
    k = 21
    fa, fq, fb, db = _files(tmp_path, k)
    ix = str(tmp_path / "ix.img")
    args = ["-hist", "-sequence", fa, "-reads", fq, "-reads", fb, "-k", str(k), "-peak", "10", "-index", ix]
    r1 = run(args + ["-output", str(tmp_path / "h1")])
    assert r1.returncode == 0 and "Writing the index image" in r1.stderr, r1.stderr
    r2 = run(args + ["-output", str(tmp_path / "h2")])
    assert r2.returncode == 0 and "Loading the index image" in r2.stderr and "rebuilding" not in r2.stderr
    st = os.stat(fb)
    os.utime(fb, ns=(st.st_atime_ns, st.st_mtime_ns + 10**9))
    r3 = run(args + ["-output", str(tmp_path / "h3")])
    assert r3.returncode == 0 and "rebuilding it" in r3.stderr and "-- Counted the 21-mers" in r3.stderr
    assert open(tmp_path / "h1", "rb").read() == open(tmp_path / "h2", "rb").read() == open(tmp_path / "h3", "rb").read()
