"""`merfin -count` end to end on the GPU: the database it writes from FASTQ / FASTA read files is byte for byte the one written from the
oracle's counts, and the modes that need every read k-mer -- -completeness, -spectrum's read-only row -- and -hist run from it as from a
`meryl print` text database of the same counts."""
import re

import pytest

from oracle import pyoracle as po
from tests import spectrum_ref
from tests import synth_reads as sr
from tests.test_cli import _write_fasta, _write_text_db, run

pytestmark = pytest.mark.gpu


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _write_fastq(path, reads):
    with open(path, "wb") as f:
        for i, s in enumerate(reads):
            f.write(b"@read%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))


def _count(tmp_path, k, reads):
    """the reads as one plain FASTQ and one .gz FASTA file through `merfin -count`; (database path, the run)"""
    half = len(reads) // 2
    fq, fa, db = str(tmp_path / "a.fastq"), str(tmp_path / "b.fasta.gz"), str(tmp_path / "reads.mfxk")
    _write_fastq(fq, [x for x in reads[:half] if x])           # (a FASTQ record has a sequence line)
    _write_fasta(fa, reads[half:], gz=True)
    r = run(["-count", "-reads", fq, "-reads", fa, "-k", str(k), "-output", db, "-min", "3", "-max", "50"])      # (-min / -max: not applied)
    assert r.returncode == 0, r.stderr
    return db, r


def _report_lines(stderr):
    return [l for l in stderr.splitlines() if l.startswith(("TOTAL", "COMPLETENESS", "thread "))]


def test_count_then_every_mode_from_the_file(tmp_path):
    m = _mfx()
    k, peak = 21, 9.0
    asm, reads = sr.reads_world(k, 1621)
    rk, rv = po.count_kmers(k, reads)
    db, r = _count(tmp_path, k, reads)
    want = str(tmp_path / "want.mfxk")
    m.db_write_flat(want, k, rk, rv)
    assert open(db, "rb").read() == open(want, "rb").read()
    assert m.db_probe(db) == {"k": k, "format": "flat", "n_kmers": len(rk)}
    assert re.search(r"-- Counted the 21-mers of \d+ reads \(%d bases\): %d k-mers, %d distinct; the table grew [1-9]\d* times? to \d+\.\d{3} GB\.\n" % (
        sum(len(x) for x in reads), int(rv.sum()), len(rk)), r.stderr), r.stderr
    assert "-- Wrote %d k-mers in " % len(rk) in r.stderr and r.stderr.rstrip().endswith("Bye!")
    txt, fa = str(tmp_path / "reads.txt"), str(tmp_path / "asm.fasta")
    _write_text_db(txt, k, rk, rv)
    _write_fasta(fa, asm)
    # -completeness: every read k-mer is walked (refused from -reads)
    a = run(["-completeness", "-sequence", fa, "-readmers", db, "-peak", str(peak)])
    b = run(["-completeness", "-sequence", fa, "-readmers", txt, "-peak", str(peak)])
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert a.stdout == b.stdout and _report_lines(a.stderr) == _report_lines(b.stderr) and len(_report_lines(a.stderr)) == 64 + 3
    # -hist, with the filter applied when the database is loaded
    for extra in ([], ["-min", "3", "-max", "50"]):
        ha = run(["-hist", "-sequence", fa, "-readmers", db, "-peak", str(peak), "-output", str(tmp_path / "a.hist")] + extra)
        hb = run(["-hist", "-sequence", fa, "-readmers", txt, "-peak", str(peak), "-output", str(tmp_path / "b.hist")] + extra)
        assert ha.returncode == 0 and hb.returncode == 0, ha.stderr + hb.stderr
        assert ha.stdout == hb.stdout and (tmp_path / "a.hist").read_bytes() == (tmp_path / "b.hist").read_bytes() and (tmp_path / "a.hist").stat().st_size > 0
    # -spectrum has its read-only row
    s = run(["-spectrum", "-sequence", fa, "-readmers", db, "-output", str(tmp_path / "s")])
    assert s.returncode == 0, s.stderr
    img = spectrum_ref.image((rk, rv), po.count_kmers(k, asm), 4, 10000)
    assert img[0].sum() > 0
    text = open(str(tmp_path / "s.spectra-cn.hist")).read()
    assert text == spectrum_ref.text(img, True) and "read-only\t" in text
    assert "Read-only k-mers: %d\n" % int(img[0].sum()) in s.stderr


def test_even_k_with_palindromes(tmp_path):
    """k = 22: a k-mer can be its own reverse complement; counted once per occurrence, as `meryl count` does"""
    m = _mfx()
    k, peak = 22, 9.0
    asm, reads = sr.reads_world(k, 1622, sizes=(9000, 4096, 500), n_reads=600)
    pal = b"ACGTTGCAAGCTTGCAACGT"                                # 20 bases; with one base on each side: 22-mers around a palindromic core
    reads = reads + [b"A" + pal + b"T", b"AATTCCGGAACCGGTTCCGGAATT" * 3, b"G" + pal + b"C"]
    rk, rv = po.count_kmers(k, reads)
    db, _ = _count(tmp_path, k, reads)
    want = str(tmp_path / "want.mfxk")
    m.db_write_flat(want, k, rk, rv)
    assert open(db, "rb").read() == open(want, "rb").read()
    txt, fa = str(tmp_path / "reads.txt"), str(tmp_path / "asm.fasta")
    _write_text_db(txt, k, rk, rv)
    _write_fasta(fa, asm)
    ha = run(["-hist", "-sequence", fa, "-readmers", db, "-peak", str(peak), "-output", str(tmp_path / "a.hist")])
    hb = run(["-hist", "-sequence", fa, "-readmers", txt, "-peak", str(peak), "-output", str(tmp_path / "b.hist")])
    assert ha.returncode == 0 and hb.returncode == 0, ha.stderr + hb.stderr
    assert ha.stdout == hb.stdout and (tmp_path / "a.hist").read_bytes() == (tmp_path / "b.hist").read_bytes() and (tmp_path / "a.hist").stat().st_size > 0
