"""`merfin -bin` end to end: the reads of a child of two haplotypes come as a .fq.gz and a .fasta file, the hap-mer sets as two flat
databases (mfx_db_write_flat) and, for one of them, as `meryl print` text; the TSV, the statistics and the split files equal, byte for
byte, the text tests/bin_ref.py formats from its sequential walk over the reads."""
import gzip
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import bin_ref as br
from tests import synth
from tests.test_cli import _write_text_db, run
from tests.test_gpu_cli_phase import _haplotype

pytestmark = pytest.mark.gpu

K = 21


def _ok(r):
    assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def trio(tmp_path_factory):
    import merfin_amd as m
    t = str(tmp_path_factory.mktemp("bin_cli"))
    r = synth.rng(5151)
    base = synth.random_contig(r, 12000).tobytes()
    mat, pat = _haplotype(r, base, 47, 11), _haplotype(r, base, 53, 29)
    mk, pk = po.count_kmers(K, [mat])[0], po.count_kmers(K, [pat])[0]
    both = np.intersect1d(mk, pk)[::40]                           # a few k-mers in both sets: shared, hits of neither
    a, b = np.union1d(np.setdiff1d(mk, pk), both), np.union1d(np.setdiff1d(pk, mk), both)
    m.db_write_flat(t + "/a.mfxk", K, a, np.ones(len(a), dtype=np.uint32))
    m.db_write_flat(t + "/b.mfxk", K, b, (1 + np.arange(len(b)) % 3).astype(np.uint32))
    _write_text_db(t + "/b.txt", K, b, (1 + np.arange(len(b)) % 3).astype(np.uint32))
    # the reads: of one parent, of the other, of both halves, of neither's markers, too short, only N, lowercase
    reads, names = [], []

    def add(x):
        names.append("read%d" % len(reads))
        reads.append(x)

    for i in range(12):
        p = int(r.integers(0, 9000))
        add((mat, pat)[i & 1][p:p + int(r.integers(200, 3000))])
    add(mat[100:600] + pat[600:1100])
    add(mat[2000:2030])                                          # one or no marker
    add(b"ACGTACGT")                                             # shorter than k
    add(b"N" * 60)
    add(pat[5000:9000].lower())
    add(b"")
    add(mat[0:11000])
    add(mat[3000:3100] + b"N" + pat[3101:3900])
    half = len(reads) // 2
    with gzip.open(t + "/r1.fq.gz", "wb") as f:                  # FASTQ: the qualities are dropped
        for n, x in zip(names[:half], reads[:half]):
            f.write(b"@%s some words\n%s\n+\n%s\n" % (n.encode(), x, b"I" * len(x)))
    with open(t + "/r2.fasta", "wb") as f:
        for n, x in zip(names[half:], reads[half:]):
            f.write(b">%s\tlength=%d\n" % (n.encode(), len(x)))
            for o in range(0, len(x), 70):
                f.write(x[o:o + 70] + b"\n")
    rows = br.counts(reads, K, a.tolist(), b.tolist())
    assert sum(x[1] for x in rows) > 500 and sum(x[2] for x in rows) > 500 and sum(x[3] for x in rows) > 10
    return {"t": t, "reads": reads, "names": names, "lens": [len(x) for x in reads], "rows": rows, "na": len(a), "nb": len(np.setdiff1d(b, a))}


def _check(w, out, ratio=1000, hits=1, rd=lambda p: open(p).read(), z="", split=False):
    cls = br.classes(w["rows"], w["na"], w["nb"], ratio, hits)
    assert rd(out + ".bin.tsv" + z) == br.format_tsv(w["names"], w["lens"], w["rows"], cls)
    assert rd(out + ".bin.stats" + z) == br.format_stats(w["lens"], w["rows"], cls, K, w["na"], w["nb"], ratio, hits)
    for c, name in enumerate((".hapA.fasta", ".hapB.fasta", ".unknown.fasta")):
        if split:
            assert rd(out + name + z) == br.format_fasta(w["names"], w["reads"], cls, c)
        else:
            assert not os.path.exists(out + name + z)
    return cls


def test_cli_bin_tsv_stats_and_split(trio):
    w, t = trio, trio["t"]
    base = ["-bin", "-reads", t + "/r1.fq.gz", "-reads", t + "/r2.fasta", "-hapmers", t + "/a.mfxk"]
    p = _ok(run(base + ["-hapmers", t + "/b.mfxk", "-output", t + "/o1", "-split"]))
    cls = _check(w, t + "/o1", split=True)
    assert set(cls) == {0, 1, 2} and cls[0] == 0 and cls[1] == 1
    lines = p.stderr.splitlines()
    for c, name in enumerate(("A", "B", "unknown")):
        sel = [i for i, x in enumerate(cls) if x == c]
        assert "-- %s: %d reads, %d bases, %d hits of A, %d of B." % (name, len(sel), sum(w["lens"][i] for i in sel), sum(w["rows"][i][1] for i in sel),
                                                                     sum(w["rows"][i][2] for i in sel)) in lines
    # the other database form, no -split: the same table
    _ok(run(base + ["-hapmers", t + "/b.txt", "-output", t + "/o2"]))
    _check(w, t + "/o2")
    # batches of 100 bases: the reads are cut across many of them
    env = dict(os.environ, MFX_BIN_BATCH="100")
    _ok(run(base + ["-hapmers", t + "/b.mfxk", "-output", t + "/o3"], env=env))
    _check(w, t + "/o3")


def test_cli_bin_ratio_minhits_and_compressed_output(trio):
    w, t = trio, trio["t"]
    base = ["-bin", "-reads", t + "/r1.fq.gz", "-reads", t + "/r2.fasta", "-hapmers", t + "/a.mfxk", "-hapmers", t + "/b.mfxk"]
    _ok(run(base + ["-output", t + "/q", "-ratio", "2.5", "-minhits", "3", "-split"]))
    cls = _check(w, t + "/q", 2500, 3, split=True)
    assert cls != br.classes(w["rows"], w["na"], w["nb"])         # the options change the classes, as the reference says
    _ok(run(base + ["-output", t + "/z.gz", "-split"]))
    _check(w, t + "/z", rd=lambda p: gzip.open(p, "rt").read(), z=".gz", split=True)
