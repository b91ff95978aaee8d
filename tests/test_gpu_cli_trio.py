"""`merfin -trio` and `merfin -histogram` end to end: three small FASTA read sets are counted with the CLI, -trio writes all its files, its
two databases equal the library's byte for byte and the ones the chain of -merge runs makes, -phase and -bin take them as -hapmers and
write what they write for the chain's; -histogram's file matches np.bincount line for line."""
import os

import numpy as np
import pytest

from tests import synth
from tests import trio_ref as tr
from tests.test_cli import _write_fasta, run
from tests.test_gpu_cli_phase import _haplotype, _ok
from tests.test_gpu_merge import _bytes

pytestmark = pytest.mark.gpu

K = 21


def _export(m, path):
    n = m.db_probe(path)["n_kmers"]
    ix = m.Index(K, n + 64)
    ix.load_db(path, 0)
    k, v, _ = ix.export()
    return k, v


def test_cli_trio_feeds_phase_and_bin(tmp_path):
    import merfin_amd as m
    r = synth.rng(5151)
    base = synth.random_contig(r, 9000).tobytes()
    mat, pat = _haplotype(r, base, 47, 11), _haplotype(r, base, 53, 29)
    t = str(tmp_path)
    for name, reads in (("mat", [mat, mat]), ("pat", [pat, pat, pat]), ("child", [mat, pat])):      # (counts of 2, 3 and 1 or 2)
        _write_fasta("%s/%s.fa" % (t, name), reads)
        _ok(run(["-count", "-reads", "%s/%s.fa" % (t, name), "-k", str(K), "-output", "%s/%s.mfxk" % (t, name)]))
    dbs = [t + "/mat.mfxk", t + "/pat.mfxk", t + "/child.mfxk"]
    # ---- explicit cutoffs: the files, against the library and against the chain of -merge runs
    p = _ok(run(["-trio", "-mat", dbs[0], "-pat", dbs[1], "-child", dbs[2], "-output", t + "/x", "-cutmat", "2", "-cutpat", "2", "-cutchild", "1"]))
    assert "-- Cutoffs: mat 2, pat 2, child 1." in p.stderr
    assert sorted(f for f in os.listdir(t) if f.startswith("x.")) == ["x.hapA.mfxk", "x.hapB.mfxk", "x.trio.stats"]      # no pass 1: no histograms, no spool
    st = m.db_trio(dbs[0], dbs[1], dbs[2], t + "/libA.mfxk", t + "/libB.mfxk", cut_mat=2, cut_pat=2, cut_child=1)
    assert _bytes(t + "/x.hapA.mfxk") == _bytes(t + "/libA.mfxk") and _bytes(t + "/x.hapB.mfxk") == _bytes(t + "/libB.mfxk")
    assert st["n_a"] > 1000 and st["n_b"] > 1000
    for own, other, hap, cut in (("mat", "pat", "A", "2"), ("pat", "mat", "B", "2")):
        _ok(run(["-merge", "%s/%s.mfxk" % (t, own), "-not", "%s/%s.mfxk" % (t, other), "-min", cut, "-output", "%s/%s.only.mfxk" % (t, own)]))
        _ok(run(["-merge", "%s/%s.only.mfxk" % (t, own), "-merge", dbs[2], "-op", "intersect", "-output", "%s/chain%s.mfxk" % (t, hap)]))
        assert _bytes("%s/chain%s.mfxk" % (t, hap)) == _bytes("%s/x.hap%s.mfxk" % (t, hap))
    stats = dict(l.split("\t") for l in open(t + "/x.trio.stats").read().splitlines())
    assert list(stats) == ["mat_kmers", "pat_kmers", "child_kmers", "both_parents", "mat_only", "pat_only", "mat_only_at_cutoff", "pat_only_at_cutoff", "child_at_cutoff",
                           "hapA_kmers", "hapB_kmers", "windows", "cut_mat", "cut_mat_auto", "cut_pat", "cut_pat_auto", "cut_child", "cut_child_auto"]
    assert [int(stats[n]) for n in ("mat_kmers", "pat_kmers", "child_kmers", "both_parents", "mat_only", "pat_only", "mat_only_at_cutoff", "pat_only_at_cutoff",
                                    "child_at_cutoff", "hapA_kmers", "hapB_kmers")] == [st[n] for n in tr.COUNTERS]
    assert (stats["cut_mat"], stats["cut_mat_auto"], stats["cut_child"], stats["cut_child_auto"]) == ("2", "0", "1", "0")
    # ---- -phase and -bin take the pair as it is, and write what they write for the chain's databases
    contigs = [mat[:4000] + pat[4000:8500], pat[1000:7000]]
    _write_fasta(t + "/asm.fa", contigs)
    _write_fasta(t + "/reads.fa", [mat[100:1300], pat[2000:3500], base[:500]])
    for which in ("x.hap", "chain"):
        a, b = ("%s/%sA.mfxk" % (t, which), "%s/%sB.mfxk" % (t, which))
        _ok(run(["-phase", "-sequence", t + "/asm.fa", "-hapmers", a, "-hapmers", b, "-output", "%s/ph_%s" % (t, which)]))
        _ok(run(["-bin", "-reads", t + "/reads.fa", "-hapmers", a, "-hapmers", b, "-output", "%s/bin_%s" % (t, which)]))
    for suffix in (".phased_block.bed", ".hapmers.count", ".phased_block.stats"):
        assert open(t + "/ph_x.hap" + suffix).read() == open(t + "/ph_chain" + suffix).read()
    assert len(open(t + "/ph_x.hap.phased_block.bed").read().splitlines()) >= 3      # (the planted switch: A then B on contig 0, B on contig 1)
    for suffix in (".bin.tsv", ".bin.stats"):
        assert open(t + "/bin_x.hap" + suffix).read() == open(t + "/bin_chain" + suffix).read()
    assert [l.split("\t")[-1] for l in open(t + "/bin_x.hap.bin.tsv").read().splitlines()[-3:-1]] == ["A", "B"]
    # ---- no child
    _ok(run(["-trio", "-mat", dbs[0], "-pat", dbs[1], "-output", t + "/y", "-cutmat", "1", "-cutpat", "1"]))
    mk, pk = _export(m, dbs[0])[0], _export(m, dbs[1])[0]
    assert np.array_equal(_export(m, t + "/y.hapA.mfxk")[0], np.setdiff1d(mk, pk)) and np.array_equal(_export(m, t + "/y.hapB.mfxk")[0], np.setdiff1d(pk, mk))


def test_cli_automatic_cutoffs_and_histogram(tmp_path):
    import merfin_amd as m
    t = str(tmp_path)
    mat, pat, child = tr.auto_world()
    names = []
    for name, (k_, v_) in (("mat", mat), ("pat", pat), ("child", child)):
        m.db_write_flat("%s/%s.mfxk" % (t, name), K, k_, v_)
        names.append("%s/%s.mfxk" % (t, name))
    p = _ok(run(["-trio", "-mat", names[0], "-pat", names[1], "-child", names[2], "-output", t + "/o", "-maxmult", "100"]))
    assert "-- Cutoffs: mat 9 (auto), pat 6 (auto), child 9 (auto)." in p.stderr
    assert sorted(f for f in os.listdir(t) if f.startswith("o.")) == ["o.child.hist", "o.hapA.mfxk", "o.hapB.mfxk", "o.mat_only.hist", "o.pat_only.hist", "o.trio.stats"]
    st = m.db_trio(names[0], names[1], names[2], t + "/libA.mfxk", t + "/libB.mfxk", cut_mat=9, cut_pat=6, cut_child=9)
    assert _bytes(t + "/o.hapA.mfxk") == _bytes(t + "/libA.mfxk") and _bytes(t + "/o.hapB.mfxk") == _bytes(t + "/libB.mfxk") and st["n_a"] > 0
    _, _, img, _ = tr.reference(mat, pat, child, 1, 1, 1, 100)

    def text(row):
        return "".join("%d\t%d\n" % (c, n) for c, n in enumerate(row.tolist()) if n)

    for r, name in enumerate(("mat_only", "pat_only", "child")):
        assert open("%s/o.%s.hist" % (t, name)).read() == text(img[r])
    stats = dict(l.split("\t") for l in open(t + "/o.trio.stats").read().splitlines())
    assert [stats[n] for n in ("cut_mat", "cut_mat_auto", "cut_pat", "cut_pat_auto", "cut_child", "cut_child_auto")] == ["9", "1", "6", "1", "9", "1"]
    # ---- -histogram: np.bincount line for line, the overflow line as -maxmult, valley and peaks on stderr
    for mm in (100, 20):
        p = _ok(run(["-histogram", names[2], "-output", "%s/c%d.hist" % (t, mm), "-maxmult", str(mm)]))
        want = np.bincount(np.minimum(child[1], mm).astype(np.int64), minlength=mm + 1)
        assert open("%s/c%d.hist" % (t, mm)).read() == text(want)
        assert "-- %d k-mers; " % len(child[0]) in p.stderr
    assert "valley 9, main_peak 25, haploid_peak 25." in run(["-histogram", names[2], "-output", t + "/again.hist", "-maxmult", "100"]).stderr
    flat = t + "/flat.mfxk"
    m.db_write_flat(flat, K, mat[0], np.ones(len(mat[0]), dtype=np.uint32))
    p = _ok(run(["-histogram", flat, "-output", t + "/flat.hist"]))       # no peak is no error here
    assert "no peak found" in p.stderr and open(t + "/flat.hist").read() == "1\t%d\n" % len(mat[0])
    # ---- ... and it is one for -trio's automatic cutoff: the database and the flag to give are named, nothing is written
    d = run(["-trio", "-mat", flat, "-pat", names[1], "-child", names[2], "-output", t + "/z", "-cutpat", "2"])
    assert d.returncode == 1 and "-trio" in d.stderr and flat in d.stderr and "-cutmat" in d.stderr, d.stderr
    assert not [f for f in os.listdir(t) if f.startswith("z.")]
