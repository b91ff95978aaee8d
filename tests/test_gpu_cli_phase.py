"""`merfin -phase` end to end: hap-mers are built with the CLI from three small FASTA read sets (-count three times, -merge mat -not pat,
-merge ... child -op intersect, both directions), -phase runs on a two-contig assembly with one planted switch, and the three files
equal, byte for byte, the text tests/phase_ref.py formats from the records expected by membership of every position's canonical k-mer."""
import gzip

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import phase_ref as pr
from tests import synth
from tests.test_cli import _write_fasta, run
from tests.test_gpu_phase import kmers_of

pytestmark = pytest.mark.gpu

K = 21


def _haplotype(r, base, every, offset):
    """the base sequence with a substitution about every `every` bases"""
    h = bytearray(base)
    for p in range(offset, len(h), every):
        h[p] = synth.BASES[(int(np.searchsorted(synth.BASES, h[p])) + int(r.integers(1, 4))) % 4]
    return bytes(h)


def _ok(r):
    assert r.returncode == 0, r.stderr
    return r


def test_cli_hapmers_and_phase_blocks(tmp_path):
    r = synth.rng(4242)
    base = synth.random_contig(r, 9000).tobytes()
    mat, pat = _haplotype(r, base, 47, 11), _haplotype(r, base, 53, 29)
    t = str(tmp_path)
    for name, reads in (("mat", [mat]), ("pat", [pat]), ("child", [mat, pat])):
        _write_fasta("%s/%s.fa" % (t, name), reads)
        _ok(run(["-count", "-reads", "%s/%s.fa" % (t, name), "-k", str(K), "-output", "%s/%s.mfxk" % (t, name)]))
    for own, other, hap in (("mat", "pat", "A"), ("pat", "mat", "B")):
        d = _ok(run(["-merge", "%s/%s.mfxk" % (t, own), "-not", "%s/%s.mfxk" % (t, other), "-output", "%s/%s.only.mfxk" % (t, own)]))
        assert "-- Subtracted: " in d.stderr
        _ok(run(["-merge", "%s/%s.only.mfxk" % (t, own), "-merge", t + "/child.mfxk", "-op", "intersect", "-output", "%s/hap%s.mfxk" % (t, hap)]))
    # what the hap-mers must be: (own - other) in the child, by the oracle's counts
    mk, pk, ck = (po.count_kmers(K, x)[0] for x in ([mat], [pat], [mat, pat]))
    a = np.intersect1d(np.setdiff1d(mk, pk), ck)
    b = np.intersect1d(np.setdiff1d(pk, mk), ck)
    import merfin_amd as m
    for hap, want in (("A", a), ("B", b)):
        ix = m.Index(K, len(want) + 64)
        ix.load_db("%s/hap%s.mfxk" % (t, hap), 0)
        np.testing.assert_array_equal(ix.export()[0], want)
    assert len(a) > 1000 and len(b) > 1000
    # the assembly: contig 0 follows the mother for 4000 bases and the father from there on (one switch), contig 1 the father
    contigs = [mat[:4000] + pat[4000:8500], pat[1000:7000]]
    names = ["ctg0", "ctg1"]
    fa = t + "/asm.fa"
    _write_fasta(fa, contigs)
    masks = []
    for c in contigs:
        v, f, rc = kmers_of(K, c)
        canon = np.minimum(f, rc)
        ina, inb = np.isin(canon, a) & v, np.isin(canon, b) & v
        masks.append((ina & ~inb, inb & ~ina, ina & inb, v))
    counts = [(int(v.sum()), int(x.sum()), int(y.sum()), int(s.sum())) for x, y, s, v in masks]
    markers = [pr.markers_of_masks(x, y) for x, y, _, _ in masks]
    for opts, S, R in (((), 100, 20000), (("-switches", "3", "-range", "500"), 3, 500)):
        want = pr.blocks(markers, K, S, R)
        out = t + "/o%d" % S
        p = _ok(run(["-phase", "-sequence", fa, "-hapmers", t + "/hapA.mfxk", "-hapmers", t + "/hapB.mfxk", "-output", out] + list(opts)))
        assert open(out + ".phased_block.bed").read() == pr.format_bed(want, names, K)
        assert open(out + ".hapmers.count").read() == pr.format_counts(counts, names)
        assert open(out + ".phased_block.stats").read() == pr.format_stats(want, K, S, R)
        # the planted switch: contig 0 is an A block, then a B block; contig 1 one B block
        assert [(x["contig"], x["hap"]) for x in want] == [(0, 0), (0, 1), (1, 1)]
        assert all(x["n_switch"] == 0 for x in want)
        lines = p.stderr.splitlines()
        for h, name in ((0, "A"), (1, "B")):
            mine = [x for x in want if x["hap"] == h]
            assert "-- %s: %d blocks, %d bases, %d markers, %d switch markers." % (
                name, len(mine), sum(x["end"] - 1 + K - x["start"] for x in mine), sum(x["n_hap"] + x["n_switch"] for x in mine), 0) in lines
        assert any(l.startswith("-- all: 3 blocks, ") and l.endswith("(switch rate 0.000000).") for l in lines)
    # a compressed -output name: the suffix moves behind the names
    _ok(run(["-phase", "-sequence", fa, "-hapmers", t + "/hapA.mfxk", "-hapmers", t + "/hapB.mfxk", "-output", t + "/z.gz"]))
    want = pr.blocks(markers, K, 100, 20000)
    assert gzip.open(t + "/z.phased_block.bed.gz", "rt").read() == pr.format_bed(want, names, K)
    assert gzip.open(t + "/z.hapmers.count.gz", "rt").read() == pr.format_counts(counts, names)
    assert gzip.open(t + "/z.phased_block.stats.gz", "rt").read() == pr.format_stats(want, K, 100, 20000)


def test_cli_phase_short_intrusion_is_a_switch_error(tmp_path):
    """a stretch of the other parent that holds two substitutions: its markers are switch markers inside the block at the defaults, a block
    of their own with -switches 0"""
    r = synth.rng(4343)
    base = synth.random_contig(r, 9000).tobytes()
    mat, pat = _haplotype(r, base, 47, 11), _haplotype(r, base, 53, 29)
    t = str(tmp_path)
    import merfin_amd as m
    mk, pk = po.count_kmers(K, [mat])[0], po.count_kmers(K, [pat])[0]
    a, b = np.setdiff1d(mk, pk), np.setdiff1d(pk, mk)
    m.db_write_flat(t + "/a.mfxk", K, a, np.ones(len(a), dtype=np.uint32))
    m.db_write_flat(t + "/b.mfxk", K, b, np.ones(len(b), dtype=np.uint32))
    contig = mat[:3000] + pat[3000:3100] + mat[3100:8000]
    _write_fasta(t + "/asm.fa", [contig])
    v, f, rc = kmers_of(K, contig)
    canon = np.minimum(f, rc)
    ina, inb = np.isin(canon, a) & v, np.isin(canon, b) & v
    markers = [pr.markers_of_masks(ina & ~inb, inb & ~ina)]
    for opts, S, R in (((), 100, 20000), (("-switches", "0"), 0, 20000)):
        want = pr.blocks(markers, K, S, R)
        _ok(run(["-phase", "-sequence", t + "/asm.fa", "-hapmers", t + "/a.mfxk", "-hapmers", t + "/b.mfxk", "-output", t + "/o"] + list(opts)))
        assert open(t + "/o.phased_block.bed").read() == pr.format_bed(want, ["ctg0"], K)
        assert open(t + "/o.phased_block.stats").read() == pr.format_stats(want, K, S, R)
        if S:
            assert len(want) == 1 and want[0]["hap"] == 0 and want[0]["n_switch"] > 0 and want[0]["n_switch_runs"] >= 1
        else:
            assert len(want) >= 3 and all(x["n_switch"] == 0 for x in want)
