"""`merfin -track`: the three files equal, byte for byte, the text a Python formatter makes from the window records expected
from the oracle's -dump values (tests/track_ref.py); the -reads run equals the -readmers run; a .gz output name round-trips;
the count lines on stderr are those of `-dump -skipMissing` on the same inputs."""
import gzip
import os

import pytest

from oracle import plain
from oracle import pyoracle as po
from tests import synth
from tests import synth_reads as sr
from tests import track_ref as tr
from tests.test_cli import _write_fasta, _write_text_db, run

pytestmark = pytest.mark.gpu


def _counts(stderr, names):
    return [l for l in stderr.splitlines() if l.split("\t")[0] in names and l.count("\t") == 3]


def _read3(prefix):
    return tuple(open(prefix + suf, "r").read() for suf in (".track.tsv", ".kstar.bedgraph", ".missing.bedgraph"))


@pytest.mark.parametrize("window", [None, 4097])
def test_cli_track_k21_files_and_counts(tmp_path, window, golden_dir):
    k, peak = 21, 26.0
    contigs, read, asm = synth.world(k=k, peak=peak, seed=77, sizes=(25000, 6000, 4096, 300, 10, 4097))
    prob = os.path.join(golden_dir, "example_lookup_table.txt")
    K, P = po.load_kmetric(prob)
    p = po.Params(k, peak, K, P)
    R, A = po.Lookup(k, *read), po.Lookup(k, *asm)
    pp = [tr.per_position_c(po, p, R, A, c) for c in contigs]
    fa = str(tmp_path / "asm.fa")
    _write_fasta(fa, contigs)
    db = str(tmp_path / "reads.txt")
    _write_text_db(db, k, *read)
    names = ["ctg%d" % i for i in range(len(contigs))]
    W = window or 1000
    want = tr.format_files(tr.reduce_windows(pp, W), names, [len(c) for c in contigs], W)
    common = ["-sequence", fa, "-readmers", db, "-peak", str(peak), "-prob", prob]
    out = str(tmp_path / "o")
    r = run(["-track"] + common + ["-output", out] + (["-window", str(window)] if window else []))
    assert r.returncode == 0, r.stderr
    assert _read3(out) == want
    d = run(["-dump", "-skipMissing"] + common + ["-output", str(tmp_path / "d")])
    assert d.returncode == 0, d.stderr
    assert _counts(r.stderr, names) == _counts(d.stderr, names) and len(_counts(r.stderr, names)) == len(contigs)
    if window:
        # a compressed -output name: the suffix moves behind the three names, the files go through the compressed writers
        z = run(["-track"] + common + ["-output", out + ".gz", "-window", str(window)])
        assert z.returncode == 0, z.stderr
        assert all(os.path.exists(out + suf + ".gz") for suf in (".track.tsv", ".kstar.bedgraph", ".missing.bedgraph"))
        assert tuple(gzip.open(out + suf + ".gz", "rt").read() for suf in (".track.tsv", ".kstar.bedgraph", ".missing.bedgraph")) == want


def test_cli_track_reads_equal_the_database_route(tmp_path):
    k = 21
    asm, reads = sr.reads_world(k, 4321)
    reads = [x for x in reads if x]
    fa = str(tmp_path / "asm.fa")
    _write_fasta(fa, asm)
    fq = str(tmp_path / "a.fq.gz")
    with gzip.open(fq, "wt") as f:
        for i, x in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, x.decode(), "I" * len(x)))
    db = str(tmp_path / "reads.txt")
    rk, rv = po.count_kmers(k, reads)
    _write_text_db(db, k, rk, rv)
    a = run(["-track", "-sequence", fa, "-reads", fq, "-k", str(k), "-peak", "10", "-window", "500", "-output", str(tmp_path / "a")])
    b = run(["-track", "-sequence", fa, "-readmers", db, "-peak", "10", "-window", "500", "-output", str(tmp_path / "b")])
    assert a.returncode == 0, a.stderr
    assert b.returncode == 0, b.stderr
    assert _read3(str(tmp_path / "a")) == _read3(str(tmp_path / "b"))
    names = ["ctg%d" % i for i in range(len(asm))]
    assert _counts(a.stderr, names) == _counts(b.stderr, names) and len(_counts(a.stderr, names)) == len(asm)
    # ... and both are the oracle's values
    p = po.Params(k, 10.0)
    R, A = po.Lookup(k, rk, rv), po.Lookup(k, *po.count_kmers(k, asm))
    pp = [tr.per_position_c(po, p, R, A, c) for c in asm]
    assert _read3(str(tmp_path / "b")) == tr.format_files(tr.reduce_windows(pp, 500), names, [len(c) for c in asm], 500)


def test_cli_track_k33(tmp_path):
    from tests.test_gpu_wide import small_world
    k, peak = 33, 9.0
    contigs, R, A = small_world(k, 833)
    contigs = [c for c in contigs if c]                          # (a FASTA record needs a base)
    pp = [tr.per_position_plain(plain, k, peak, [], [], c, R, A) for c in contigs]
    fa = str(tmp_path / "asm.fa")
    _write_fasta(fa, [c.encode() for c in contigs])
    db = str(tmp_path / "reads.txt")
    with open(db, "w") as f:
        for x in sorted(R):
            f.write("%s\t%d\n" % (plain.dec(x, k), R[x]))
    names = ["ctg%d" % i for i in range(len(contigs))]
    W = 777
    r = run(["-track", "-sequence", fa, "-readmers", db, "-peak", str(peak), "-window", str(W), "-output", str(tmp_path / "o")])
    assert r.returncode == 0, r.stderr
    assert _read3(str(tmp_path / "o")) == tr.format_files(tr.reduce_windows(pp, W), names, [len(c) for c in contigs], W)
    d = run(["-dump", "-skipMissing", "-sequence", fa, "-readmers", db, "-peak", str(peak), "-output", str(tmp_path / "d")])
    assert d.returncode == 0, d.stderr
    assert _counts(r.stderr, names) == _counts(d.stderr, names) and len(_counts(r.stderr, names)) == len(contigs)
