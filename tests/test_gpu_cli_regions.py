"""`merfin -regions`: <out>.regions.bed equals, byte for byte, the text tests/regions_ref.py formats from the records expected from
the oracle's -dump values, from FASTA plus a flat `.mfxk` database (the form `merfin` stages into device memory from process start) and
from a `meryl print` text database; the -reads run equals the -readmers run; a .gz output name round-trips; the count lines on stderr are
those of `-dump -skipMissing`, the summary lines count the file's records; -peak auto writes the file of the peak it reports."""
import gzip
import os
import re

import pytest

from oracle import pyoracle as po
from tests import regions_ref as rr
from tests import synth
from tests import synth_reads as sr
from tests import track_ref as tr
from tests.test_cli import _write_fasta, _write_text_db, run

pytestmark = pytest.mark.gpu


def _counts(stderr, names):
    return [l for l in stderr.splitlines() if l.split("\t")[0] in names and l.count("\t") == 3]


def _summary(recs, k):
    out = []
    for cls, name in enumerate(rr.CLASSES):
        mine = recs[recs["cls"] == cls]
        out.append("-- %s: %d regions, %d flagged k-mers, %d bases covered." % (name, len(mine), int(mine["n_kmers"].sum()),
                                                                                  int((mine["end"] - 1 + k - mine["start"]).sum())))
    return out


@pytest.mark.parametrize("form", ["mfxk", "text"])
@pytest.mark.parametrize("opts", [(), ("-kstar", "0.5", "-gap", "20", "-minrun", "21")])
def test_cli_regions_k21_file_counts_and_summary(tmp_path, opts, form, golden_dir):
    k, peak = 21, 26.0
    contigs, read, asm = synth.world(k=k, peak=peak, seed=77, sizes=(25000, 6000, 4096, 300, 10, 4097))
    prob = os.path.join(golden_dir, "example_lookup_table.txt")
    K, P = po.load_kmetric(prob)
    p = po.Params(k, peak, K, P)
    R, A = po.Lookup(k, *read), po.Lookup(k, *asm)
    pp = [tr.per_position_c(po, p, R, A, c) for c in contigs]
    fa = str(tmp_path / "asm.fa")
    _write_fasta(fa, contigs)
    if form == "mfxk":                                         # the sorted flat database: the staged load of the sequence-only build
        import merfin_amd as m
        db = str(tmp_path / "reads.mfxk")
        m.db_write_flat(db, k, *read)
        assert m.db_probe(db)["format"] == "flat"
    else:
        db = str(tmp_path / "reads.txt")
        _write_text_db(db, k, *read)
    names = ["ctg%d" % i for i in range(len(contigs))]
    t, gap, mk = (0.5, 20, 21) if opts else (1.0, 0, 1)
    recs = rr.regions(pp, t, gap, mk)
    want = rr.format_bed(recs, names, k)
    assert want.count("\n") > 10
    common = ["-sequence", fa, "-readmers", db, "-peak", str(peak), "-prob", prob]
    out = str(tmp_path / "o")
    r = run(["-regions"] + common + ["-output", out] + list(opts))
    assert r.returncode == 0, r.stderr
    assert open(out + ".regions.bed").read() == want
    d = run(["-dump", "-skipMissing"] + common + ["-output", str(tmp_path / "d")])
    assert d.returncode == 0, d.stderr
    assert _counts(r.stderr, names) == _counts(d.stderr, names) and len(_counts(r.stderr, names)) == len(contigs)
    lines = r.stderr.splitlines()
    s = _summary(recs, k)
    at = lines.index(s[0])
    assert lines[at:at + 3] == s and at > lines.index(_counts(r.stderr, names)[-1])      # behind the count lines
    if opts:
        # a compressed -output name: the suffix moves behind the name, the file goes through the compressed writer
        z = run(["-regions"] + common + ["-output", out + ".gz"] + list(opts))
        assert z.returncode == 0, z.stderr
        assert gzip.open(out + ".regions.bed.gz", "rt").read() == want


def test_cli_regions_reads_equal_the_database_route(tmp_path):
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
    a = run(["-regions", "-sequence", fa, "-reads", fq, "-k", str(k), "-peak", "10", "-kstar", "0.5", "-output", str(tmp_path / "a")])
    b = run(["-regions", "-sequence", fa, "-readmers", db, "-peak", "10", "-kstar", "0.5", "-output", str(tmp_path / "b")])
    assert a.returncode == 0, a.stderr
    assert b.returncode == 0, b.stderr
    ta, tb = open(str(tmp_path / "a.regions.bed")).read(), open(str(tmp_path / "b.regions.bed")).read()
    assert ta == tb
    names = ["ctg%d" % i for i in range(len(asm))]
    assert _counts(a.stderr, names) == _counts(b.stderr, names) and len(_counts(a.stderr, names)) == len(asm)
    # ... and both are the oracle's values
    p = po.Params(k, 10.0)
    R, A = po.Lookup(k, rk, rv), po.Lookup(k, *po.count_kmers(k, asm))
    pp = [tr.per_position_c(po, p, R, A, c) for c in asm]
    assert tb == rr.format_bed(rr.regions(pp, 0.5, 0, 1), names, k) and tb.count("\n") > 1


def test_cli_regions_peak_auto_is_the_explicit_peak_it_reports(tmp_path):
    k, peak = 21, 26.0
    contigs, read, asm = synth.world(k=k, peak=peak, seed=78, sizes=(60000, 6000, 4097))
    fa = str(tmp_path / "asm.fa")
    _write_fasta(fa, contigs)
    import merfin_amd as m
    db = str(tmp_path / "reads.mfxk")
    m.db_write_flat(db, k, *read)
    a = run(["-regions", "-sequence", fa, "-readmers", db, "-peak", "auto", "-output", str(tmp_path / "a")])
    assert a.returncode == 0, a.stderr
    found = re.search(r"^Haploid peak \(auto\): (\d+)  \(main peak ", a.stderr, re.M)
    assert found, a.stderr
    b = run(["-regions", "-sequence", fa, "-readmers", db, "-peak", found.group(1), "-output", str(tmp_path / "b")])
    assert b.returncode == 0, b.stderr
    text = open(str(tmp_path / "a.regions.bed")).read()
    assert text == open(str(tmp_path / "b.regions.bed")).read() and text.count("\n") > 1
