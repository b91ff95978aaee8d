"""Evaluator.regions / mfx_regions_run: maximal runs of missing, collapsed and expanded k-mers as intervals, made on the device.  The
expected records are the per-position values of the oracle's -dump (oracle.pyoracle.process_dump; the plain-Python restatement
oracle/plain.py for 32 <= k <= 64) taken through the numpy pipeline of tests/regions_ref.py -- class arrays, runs by np.diff, the
joining over gaps, the filter, the sums.  EVERY field of EVERY record is compared with `==`: there is no tolerance anywhere."""
import gzip
import os

import numpy as np
import pytest

from oracle import plain
from oracle import pyoracle as po
from tests import regions_ref as rr
from tests import synth
from tests import track_ref as tr
from tests.test_gpu_parity import build_index
from tests.test_gpu_seqonly import seq_index
from tests.test_gpu_wide import small_world, build as build_wide

pytestmark = pytest.mark.gpu

SIZES = (120000, 9000, 4096, 4097, 500, 20, 10, 0, 8191)       # > 100 000, shorter than k, empty, one position past a tile
KSTARS = (0.2, 0.5, 1.0, 1e9)


def gaps_of(k):
    return (0, 1, k - 1, 64, 4096, 10**6)


def mins_of(k):
    return (1, k, 1000)


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _prob(golden_dir, use_prob):
    return po.load_kmetric(os.path.join(golden_dir, "example_lookup_table.txt")) if use_prob else (None, None)


def _per_position(k, peak, probK, probP, contigs, read, asm):
    p = po.Params(k, peak, probK, probP)
    R, A = po.Lookup(k, *read), po.Lookup(k, *asm)
    return [tr.per_position_c(po, p, R, A, c) for c in contigs]


def canon_at(k, contig, positions):
    """the canonical k-mers starting at these positions (2 bits a base: (c >> 1) & 3, first base in the highest bits)"""
    out = []
    for p in positions:
        f = 0
        for ch in contig[p:p + k]:
            assert chr(ch) in "ACGTacgt", (p, ch)
            f = (f << 2) | ((ch >> 1) & 3)
        out.append(po.lib().orc_canonical(f, k))
    return np.array(out, dtype=np.uint64)


def drop(read, kmers):
    keep = ~np.isin(read[0], kmers)
    return read[0][keep], read[1][keep]


def _check(m, ev, seqs, pp, k, kstars=KSTARS, gaps=None, mins=None):
    """every threshold, gap and filter: records == the reference's; totals == -hist's; the missing regions hold kmissing k-mers; a
    second run is byte-identical; pass 2 visits no tile without a flagged position.  Returns the reference at gap 0, filter 1 per threshold."""
    h = ev.hist(seqs)
    base = {}
    for t in kstars:
        masks = rr.masks_of(pp, t)
        flagged = rr.flagged_tiles(masks)
        for gap in (gaps or gaps_of(k)):
            for mk in (mins or mins_of(k)):
                want = rr.regions(pp, t, gap, mk, masks)
                got, kasm, kmissing, revisited = ev.regions(seqs, t, gap, mk)
                assert got.dtype == m.REGION_DTYPE and got.dtype.itemsize == 56
                assert rr.same_records(got, want) is None, (t, gap, mk, rr.same_records(got, want))
                assert (kasm, kmissing) == (h.kasm, h.kmissing), (t, gap, mk)
                assert revisited <= flagged, (t, gap, mk, revisited, flagged)
                assert revisited == (flagged if len(want) else 0)
                again = ev.regions(seqs, t, gap, mk)[0]
                assert got.tobytes() == again.tobytes(), (t, gap, mk)
                if gap == 0 and mk == 1:
                    assert int(got["n_kmers"][got["cls"] == 0].sum(dtype=np.uint64)) == h.kmissing, t
                    base[t] = want
    assert h.kasm > 0
    return base


@pytest.mark.parametrize("use_prob", [False, True])
@pytest.mark.parametrize("index", ["full", "seq"])
@pytest.mark.parametrize("k", [15, 21, 22, 31])
def test_regions_match_the_reduced_dump(k, index, use_prob, golden_dir):
    m = _mfx()
    peak = 26.0 if use_prob else 17.3
    probK, probP = _prob(golden_dir, use_prob)
    contigs, read, asm = synth.world(k=k, peak=peak, seed=7000 + k, sizes=SIZES)
    pp = _per_position(k, peak, probK, probP, contigs, read, asm)
    if index == "full":
        ix, seqs = build_index(m, k, read, asm), m.Sequences(contigs)
    else:
        ix, seqs = seq_index(m, k, contigs, read)
        assert ix.info()["compact"]
    ev = m.Evaluator(ix, m.KParams(peak, probK, probP))
    base = _check(m, ev, seqs, pp, k)
    for t in (0.2, 0.5, 1.0):
        assert set(base[t]["cls"].tolist()) == {0, 1, 2}, t   # every class has a region
    assert any(((km == 1.0) & valid & (rk == 2) & (ak == 1)).any() for valid, rk, ak, km in pp)     # K* == t exactly: equality is in
    assert len(base[1e9]) and set(base[1e9]["cls"].tolist()) == {0}
    # the records do not depend on the form the sequence is held in: the packed planes give the same bytes
    before = {(t, g): ev.regions(seqs, t, g, 1)[0].tobytes() for t in (0.5, 1.0) for g in (0, k - 1)}
    seqs.pack()
    for (t, g), b in before.items():
        assert ev.regions(seqs, t, g, 1)[0].tobytes() == b, (t, g)


def _boundary_world(k, peak):
    """SIZES with the read k-mers removed that start on the wave, round and tile edges of contig 0, at the end of contig 1 and the start
    of contig 2, and on both sides of contig 1's N run"""
    contigs, read, asm = synth.world(k=k, peak=peak, seed=7100, sizes=SIZES)
    c0, c1, c2 = contigs[0], contigs[1], contigs[2]
    b1 = np.frombuffer(c1, dtype=np.uint8) & 0xDF
    isn = np.flatnonzero(b1 == ord("N"))
    d = np.diff(isn)
    # the N run of decorate(): 200 consecutive N
    brk = np.flatnonzero(d != 1)
    groups = np.split(isn, brk + 1)
    run = max(groups, key=len)
    n0, n1 = int(run[0]), int(run[-1]) + 1
    assert n1 - n0 >= 200
    before = list(range(n0 - k - 3, n0 - k + 1))               # the last four k-mer starts in front of the N run
    after = list(range(n1, n1 + 4))                            # the first four behind it
    last1 = list(range(len(c1) - k - 6, len(c1) - k + 1))      # the last seven k-mer starts of contig 1
    kill = [canon_at(k, c0, list(range(0, 5)) + list(range(60, 70)) + list(range(250, 262)) + list(range(4090, 4100))),
            canon_at(k, c1, before + after + last1), canon_at(k, c2, [0, 1, 2])]
    return contigs, drop(read, np.concatenate(kill)), asm, (n0, n1, before, after, last1)


def _covers(recs, contig, a, b, cls=0):
    """a record of the class on the contig that holds the positions a and b"""
    return any(r["contig"] == contig and r["cls"] == cls and r["start"] <= a and b < r["end"] for r in recs)


@pytest.mark.parametrize("index", ["full", "seq"])
def test_regions_on_wave_round_tile_and_contig_boundaries(index):
    m = _mfx()
    k, peak = 21, 17.3
    contigs, read, asm, (n0, n1, before, after, last1) = _boundary_world(k, peak)
    pp = _per_position(k, peak, None, None, contigs, read, asm)
    if index == "full":
        ix, seqs = build_index(m, k, read, asm), m.Sequences(contigs)
    else:
        ix, seqs = seq_index(m, k, contigs, read)
    ev = m.Evaluator(ix, m.KParams(peak))
    masks = rr.masks_of(pp, 1.0)
    ref0 = rr.device_records(rr.regions(pp, 1.0, 0, 1, masks))
    assert _covers(ref0, 0, 0, 4) and _covers(ref0, 0, 63, 64) and _covers(ref0, 0, 255, 256) and _covers(ref0, 0, 4095, 4096)
    for gap in gaps_of(k):
        ref = rr.device_records(rr.regions(pp, 1.0, gap, 1, masks))
        # a run ends contig 1 while contig 2 starts flagged: two records at every gap
        tail = [r for r in ref if r["contig"] == 1 and r["cls"] == 0 and r["end"] == len(contigs[1]) - k + 1]
        head = [r for r in ref if r["contig"] == 2 and r["cls"] == 0 and r["start"] == 0]
        assert len(tail) == 1 and len(head) == 1, gap
        # the N run: k - 1 + its length positions lie between the runs on its two sides
        bridged = _covers(ref, 1, before[-1], after[0])
        assert bridged == (gap >= (n1 - n0) + k - 1), gap
        assert _covers(ref, 1, before[0], before[-1]) and _covers(ref, 1, after[0], after[-1])
    assert (n1 - n0) + k - 1 <= 4096
    _check(m, ev, seqs, pp, k, kstars=(1.0,))


def test_regions_many_one_position_runs():
    """every second position's k-mer of the 9000-base contig is missing from the reads: thousands of runs, one region per stretch at gap 1"""
    m = _mfx()
    k, peak = 21, 17.3
    contigs, read, asm = synth.world(k=k, peak=peak, seed=7200, sizes=SIZES)
    valid = tr.valid_starts(contigs[1], k)
    even = [p for p in range(0, len(contigs[1]), 2) if valid[p]]
    read = drop(read, canon_at(k, contigs[1], even))
    pp = _per_position(k, peak, None, None, contigs, read, asm)
    masks = rr.masks_of(pp, 1.0)
    on1 = lambda recs: recs[(recs["contig"] == 1) & (recs["cls"] == 0)]
    gap0, gap1 = on1(rr.regions(pp, 1.0, 0, 1, masks)), on1(rr.regions(pp, 1.0, 1, 1, masks))
    assert len(gap0) > 2000
    # gap 1: exactly one region in every stretch of valid k-mers that holds an even position (its even positions are all missing and lie
    # two apart; the invalid positions between two stretches are k at the least, so nothing joins across them), none anywhere else
    # unless a stretch of odd positions only is missing by itself
    a, b = rr.runs(valid)
    assert len(a) > 3
    total = 0
    for s0, e0 in zip(a.tolist(), b.tolist()):
        inside = int(((gap1["start"] >= s0) & (gap1["end"] <= e0)).sum())
        has_even = any(p % 2 == 0 for p in range(s0, min(e0, s0 + 2)))
        assert inside == 1 if has_even else inside <= 1, (s0, e0, inside)
        total += inside
    assert total == len(gap1)
    ix, seqs = seq_index(m, k, contigs, read)
    _check(m, m.Evaluator(ix, m.KParams(peak)), seqs, pp, k, kstars=(1.0,))


def test_regions_all_and_none(tmp_path):
    m = _mfx()
    k, peak = 21, 10.0
    contigs, read, asm = synth.world(k=k, peak=peak, seed=7300, sizes=SIZES)
    names = ["c%d" % i for i in range(len(contigs))]
    # a foreign read table: every valid k-mer is missing -- one region per valid stretch
    _, foreign, _ = synth.world(k=k, peak=peak, seed=7301, sizes=(20000,))
    assert not np.isin(foreign[0], asm[0]).any()
    pp = _per_position(k, peak, None, None, contigs, foreign, asm)
    ix, seqs = seq_index(m, k, contigs, foreign)
    ev = m.Evaluator(ix, m.KParams(peak))
    base = _check(m, ev, seqs, pp, k, kstars=(1.0,), gaps=(0, k - 1), mins=(1, k))
    stretches = sum(len(rr.runs(x[0])[0]) for x in pp)
    assert len(base[1.0]) == stretches > len(contigs) and set(base[1.0]["cls"].tolist()) == {0}
    got = ev.regions(seqs, 1.0)[0]
    m.regions_write(got, seqs, names, k, str(tmp_path / "all.bed.gz"))
    assert gzip.open(tmp_path / "all.bed.gz", "rt").read() == rr.format_bed(base[1.0], names, k)
    # a read table that is the assembly's counts times the peak: K* == 0 everywhere, no record
    same = (asm[0], (asm[1].astype(np.uint64) * 10).astype(np.uint32))
    pp = _per_position(k, peak, None, None, contigs, same, asm)
    ix, seqs = seq_index(m, k, contigs, same)
    ev = m.Evaluator(ix, m.KParams(peak))
    base = _check(m, ev, seqs, pp, k, kstars=(0.2, 1.0), gaps=(0, 4096), mins=(1,))
    assert len(base[0.2]) == 0
    got, _, kmissing, revisited = ev.regions(seqs, 0.2)
    assert len(got) == 0 and got.dtype == m.REGION_DTYPE and kmissing == 0 and revisited == 0
    m.regions_write(got, seqs, names, k, str(tmp_path / "none.bed"))
    assert (tmp_path / "none.bed").read_text() == rr.HEADER


def test_regions_non_canonical_database():
    """a database of forward-strand k-mers: both strands are probed and summed (merfin-globals.C:107-108)"""
    m = _mfx()
    k = 11
    r = synth.rng(3)
    contigs = synth.as_bytes(synth.decorate(r, synth.make_truth(r, (60000, 2500, 4097, 5, 0))))
    fw = {}
    for c in contigs:
        for _, f, _r in po.kiter(k, c):
            fw[f] = fw.get(f, 0) + 1
    ak = np.array(sorted(fw), dtype=np.uint64)
    av = np.array([fw[x] for x in ak.tolist()], dtype=np.uint32)
    rv = (av * 5 + (ak % 3).astype(np.uint32)).astype(np.uint32)
    rv[ak % 7 == 0] = 0
    ix = build_index(m, k, (ak, rv), (ak, av))
    assert not ix.info()["canonical"]
    pp = _per_position(k, 5.0, None, None, contigs, (ak, rv), (ak, av))
    base = _check(m, m.Evaluator(ix, m.KParams(5.0)), m.Sequences(contigs), pp, k, kstars=(0.2, 1.0), gaps=(0, k - 1, 4096), mins=(1, k))
    assert len(base[0.2])


@pytest.mark.parametrize("k", [6, 22])
def test_regions_even_k_palindromes(k):
    m = _mfx()
    contigs, read, asm = synth.world(k=k, peak=3.0, sizes=(30000, 700, 4100, 3, 0), err_kmers=0, tandem=None, seed=31 + k)
    pp = _per_position(k, 3.0, None, None, contigs, read, asm)
    base = _check(m, m.Evaluator(build_index(m, k, read, asm), m.KParams(3.0)), m.Sequences(contigs), pp, k, kstars=(0.5, 1.0), gaps=(0, k - 1, 64),
                  mins=(1, k))
    assert len(base[0.5])


@pytest.mark.parametrize("index", ["full", "seq"])
def test_regions_foreign_assembly_database_leaves_nonfinite_out(index):
    """-seqmers of another assembly: k-mers of the sequence with asmV == 0, where getKmetric divides by zero -- in no class"""
    m = _mfx()
    k, peak = 21, 17.3
    contigs, read, asm = synth.world(k=k, peak=peak, seed=909, sizes=SIZES)
    keep = np.random.default_rng(5).random(len(asm[0])) < 0.9
    foreign = (asm[0][keep], asm[1][keep])
    pp = _per_position(k, peak, None, None, contigs, read, foreign)
    assert any((valid & (rk != 0) & (ak == 0)).any() for valid, rk, ak, km in pp)
    if index == "full":
        ix, seqs = build_index(m, k, read, foreign), m.Sequences(contigs)
    else:
        ix, seqs = seq_index(m, k, contigs, read, foreign)
    _check(m, m.Evaluator(ix, m.KParams(peak)), seqs, pp, k, kstars=(0.5, 1e9), gaps=(0, k - 1, 4096), mins=(1, k))


@pytest.mark.parametrize("k,use_prob", [(33, False), (33, True), (64, False), (64, True)])
def test_regions_wide_kmers(k, use_prob, golden_dir):
    m = _mfx()
    peak = 9.0
    probK, probP = _prob(golden_dir, use_prob)
    pk, ppb = (probK.tolist(), probP.tolist()) if use_prob else ([], [])
    contigs, R, A = small_world(k, 800 + k)
    pp = [tr.per_position_plain(plain, k, peak, pk, ppb, c, R, A) for c in contigs]
    ix = build_wide(m, k, R, A)
    ev = m.Evaluator(ix, m.KParams(peak, probK, probP))
    base = _check(m, ev, m.Sequences([c.encode() for c in contigs]), pp, k, kstars=(0.2, 1.0, 1e9), gaps=(0, k - 1, 4096), mins=(1, k))
    assert len(base[0.2])


def test_regions_refusals_and_text(tmp_path):
    m = _mfx()
    k, peak = 21, 17.3
    contigs, read, asm = synth.world(k=k, peak=peak, seed=12, sizes=(9000, 4097, 10, 0))
    seqs = m.Sequences(contigs)
    ix = build_index(m, k, read, asm)
    ev = m.Evaluator(ix, m.KParams(peak))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(m.MfxError) as e:
            ev.regions(seqs, bad)
        assert e.value.code == -1 and "-kstar must be a finite number above 0" in str(e.value), bad
    # the text: the formatter of the expected records, byte for byte; a .gz name goes through the compressed writer
    names = ["c%d" % i for i in range(len(contigs))]
    pp = _per_position(k, peak, None, None, contigs, read, asm)
    for t, gap, mk in ((1.0, 0, 1), (0.5, k - 1, k)):
        got = ev.regions(seqs, t, gap, mk)[0]
        text = rr.format_bed(rr.regions(pp, t, gap, mk), names, k)
        assert text.count("\n") > 3
        m.regions_write(got, seqs, names, k, str(tmp_path / "r.bed"))
        m.regions_write(got, seqs, names, k, str(tmp_path / "r.bed.gz"))
        assert (tmp_path / "r.bed").read_text() == text and gzip.open(tmp_path / "r.bed.gz", "rt").read() == text
    bad = got.copy()
    bad["end"][0] = len(contigs[0]) + 5                        # a record that is no region of these sequences
    with pytest.raises(m.MfxError):
        m.regions_write(bad, seqs, names, k, str(tmp_path / "x.bed"))
    # a shard of an index cannot answer for a k-mer's class
    sx = m.Index(k, len(read[0]) + len(asm[0]) + 16)
    sx.set_shard(0, 2)
    sx.add_read(*read)
    sx.add_asm(*asm)
    with pytest.raises(m.MfxError) as e:
        m.Evaluator(sx, m.KParams(peak)).regions(seqs)
    assert e.value.code == -1 and "shard" in str(e.value)
