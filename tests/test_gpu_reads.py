"""The read k-mer counter (mfx_reads_begin / add / end, Index.count_reads): the read counts of a run straight from its reads,
counted on the device into the k-mers a sequence-only or path-only index claimed.  The table must be the one a database of
those reads gives (`meryl count` semantics: canonical k-mers, all k bases ACGT in either case), restricted to the claimed
k-mers -- exactly, in every layout, whatever the batching, with counts past the compact layout's 2047 and past 65535."""
import numpy as np
import pytest

from oracle import plain
from oracle import pyoracle as po
from tests import synth, synth_reads as sr
from tests.test_cli import _write_text_db
from tests.test_gpu_parity import assert_hist_equal, oracle_hist

pytestmark = pytest.mark.gpu


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _expected(k, asm, reads):
    """(asm k-mers, asm counts, read counts of those k-mers, all read k-mers, their counts)"""
    ak, av = po.count_kmers(k, asm)
    rk, rv = po.count_kmers(k, reads)
    i = np.searchsorted(rk, ak)
    i[i >= len(rk)] = 0
    er = np.where((len(rk) > 0) & (rk[i] == ak), rv[i], 0).astype(np.uint32)
    return ak, av, er, rk, rv


def _seq_index(m, k, asm, seqs=None):
    seqs = seqs or m.Sequences(asm)
    ix = m.Index.for_seq(k, sum(len(c) for c in asm) + 16)
    ix.count_asm(seqs)
    return ix, seqs


LOW_COMPLEXITY_CONTIGS = [b"A" * 200, b"TTAGGG" * 40, b"CCCTA" * 40, b"AC" * 100, b"C" * 200]


@pytest.mark.parametrize("k,compact", [(15, "1"), (20, "1"), (21, "1"), (22, "1"), (31, "1"), (21, "0"), (31, "0")])
def test_counts_equal_the_oracle_and_the_database_route(k, compact, tmp_path, monkeypatch):
    m = _mfx()
    monkeypatch.setenv("MFX_SEQ_COMPACT", compact)
    peak = 9.0
    asm, reads = sr.reads_world(k, 700 + k)
    ak, av, er, rk, rv = _expected(k, asm, reads)
    ix, seqs = _seq_index(m, k, asm)
    assert ix.info()["compact"] == (compact == "1")
    st = ix.count_reads(reads)
    ek, erv, eav = ix.export()
    np.testing.assert_array_equal(ek, ak)
    np.testing.assert_array_equal(erv, er)
    np.testing.assert_array_equal(eav, av)
    assert st["reads"] == len(reads) and st["bases"] == sum(len(x) for x in reads)
    assert st["kmers"] == int(rv.sum()) and st["counted"] == int(er.sum()) and st["dropped"] == st["kmers"] - st["counted"]
    assert st["dropped"] > 0 and st["saturated"] == 0
    # the same index through a `meryl print` text database of all read k-mers
    db = str(tmp_path / "reads.txt")
    _write_text_db(db, k, rk, rv)
    ix2, _ = _seq_index(m, k, asm, seqs)
    ix2.load_db(db, 0)
    for a, b in zip(ix2.export(), (ek, erv, eav)):
        np.testing.assert_array_equal(a, b)
    # -hist and -dump: bit-identical between the two routes and against the oracle
    p, g, ka, km = oracle_hist(k, peak, asm, (rk, rv), (ak, av))
    dumps = []
    for x in (ix, ix2):
        ev = m.Evaluator(x, m.KParams(peak))
        assert_hist_equal(ev.hist(seqs), g, ka, km, k)
        dumps.append(ev.dump_values(seqs, 0, 0, len(asm[0]) - k + 1))
    for a, b in zip(dumps[0], dumps[1]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("k", [21, 31])
def test_batching_and_order_do_not_matter(k):
    """batches small enough to split most reads (k-1 overlap), and the reads shuffled: the same table"""
    m = _mfx()
    asm, reads = sr.reads_world(k, 800 + k, n_reads=1500)
    ak, av, er, _, rv = _expected(k, asm, reads)
    ref = None
    for bb, rs in ((0, reads), (2 * k + 3, reads), (97, list(reversed(reads))), (1000, [reads[i] for i in synth.rng(3).permutation(len(reads))])):
        ix, _ = _seq_index(m, k, asm)
        st = ix.count_reads(rs, batch_bases=bb, chunk=333)
        got = ix.export()
        np.testing.assert_array_equal(got[1], er)
        assert st["kmers"] == int(rv.sum())
        if ref is not None:
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a, b)
        ref = got


@pytest.mark.parametrize("k,compact", [(21, "1"), (31, "1"), (21, "0")])
def test_saturation_and_contention(k, compact, monkeypatch):
    """homopolymers, (TTAGGG)n and a 5-mer tandem array: counts past 2047 (the compact field moves to the side table) and past 65535"""
    m = _mfx()
    monkeypatch.setenv("MFX_SEQ_COMPACT", compact)
    asm, reads = sr.reads_world(k, 900 + k, n_reads=800)
    asm = asm + LOW_COMPLEXITY_CONTIGS
    reads = reads + sr.low_complexity_reads(synth.rng(17), n_each=500)
    ak, av, er, rk, rv = _expected(k, asm, reads)
    assert er.max() > 65535 and np.count_nonzero(er > 2047) >= 5
    ix, seqs = _seq_index(m, k, asm)
    st = ix.count_reads(reads, batch_bases=5000)
    ek, erv, eav = ix.export()
    np.testing.assert_array_equal(ek, ak)
    np.testing.assert_array_equal(erv, er)
    np.testing.assert_array_equal(eav, av)
    if compact == "1":
        assert st["saturated"] == int(np.count_nonzero(er >= 2047))
    # -min / -max apply to the counted table as to a loaded one
    lo, hi = 3, 5000
    ix2, _ = _seq_index(m, k, asm, seqs)
    ix2.count_reads(reads, minV=lo, maxV=hi)
    peak = 12.0
    _, g, ka, km = oracle_hist(k, peak, asm, (rk, rv), (ak, av), minV=lo, maxV=hi)
    assert_hist_equal(m.Evaluator(ix2, m.KParams(peak)).hist(seqs), g, ka, km, k)


def _key128(lo, hi):
    return [int(a) | (int(b) << 64) for a, b in zip(lo, hi)]


@pytest.mark.parametrize("k", [33, 64])
def test_wide_k_on_the_plain_oracle(k):
    """32 <= k <= 64: the table of the assembly's k-mers (mfx_wide.hip), counted per lane"""
    m = _mfx()
    asm, reads = sr.reads_world(k, 950 + k, sizes=(900, 400), n_reads=250, lens=(40, 200))
    seqs = m.Sequences(asm)
    ix = m.Index(k, 4096)
    ix.count_asm(seqs)
    st = ix.count_reads(reads, batch_bases=301)
    ek, erv, eav = ix.export()
    want_a = plain.count_kmers(k, [c.decode() for c in asm])
    want_r = plain.count_kmers(k, [x.decode() for x in reads])
    keys = _key128(ek[:, 0], ek[:, 1])
    assert sorted(keys) == sorted(want_a)
    assert [int(x) for x in erv] == [want_r.get(x, 0) for x in keys]
    assert [int(x) for x in eav] == [want_a[x] for x in keys]
    assert st["kmers"] == sum(want_r.values()) and st["counted"] == sum(want_r.get(x, 0) for x in keys)


@pytest.mark.parametrize("mode", ["polish", "filter"])
@pytest.mark.parametrize("k", [21, 31])
def test_variant_modes_on_the_path_only_index(tmp_path, mode, k):
    """-polish / -filter from reads counted into the path-only index: the records of the oracle and of the database route on the full tables"""
    m = _mfx()
    peak = 9.0
    names, asm, vcf, truth = synth.variant_world(k=k, peak=peak, seed=60 + k, tables=False)
    vp = str(tmp_path / "in.vcf")
    open(vp, "w").write(vcf)
    reads = sr.sample_reads(synth.rng(61 + k), truth, 700, k, lens=(80, 300))
    ak, av = po.count_kmers(k, asm)
    rk, rv = po.count_kmers(k, reads)
    ix = m.Index(k, len(rk) + len(ak) + 16)
    ix.add_read(rk, rv)
    ix.add_asm(ak, av)
    n_a = m.Evaluator(ix, m.KParams(peak)).variants(mode, vp, names, asm, str(tmp_path / "a.vcf"), log_path=str(tmp_path / "a.log"))
    loaded = m.LoadedVcf(vp)
    px = loaded.prepare_path_index(k, mode, names, asm)
    assert px is not None
    px.add_asm(ak, av)
    st = px.count_reads(reads)
    assert st["counted"] > 0 and st["dropped"] > 0
    n_b = m.Evaluator(px, m.KParams(peak)).variants_loaded(mode, loaded, names, asm, str(tmp_path / "b.vcf"), log_path=str(tmp_path / "b.log"))
    n_o = po.variants_run(po.Params(k, peak), po.Lookup(k, rk, rv), po.Lookup(k, ak, av), mode, vp, names, asm, str(tmp_path / "o.vcf"),
                          log_path=str(tmp_path / "o.log"))
    assert n_a == n_b == n_o and n_a > 0
    assert open(tmp_path / "a.vcf", "rb").read() == open(tmp_path / "b.vcf", "rb").read() == open(tmp_path / "o.vcf", "rb").read()
    assert open(tmp_path / "a.log", "rb").read() == open(tmp_path / "b.log", "rb").read()      # (the oracle's log holds its special lines only)
    loaded.close()


def test_refusals():
    m = _mfx()
    k = 21
    asm, reads = sr.reads_world(k, 990, sizes=(3000,), n_reads=50)
    seqs = m.Sequences(asm)
    # a full index
    full = m.Index(k, 10000)
    with pytest.raises(m.MfxError) as e:
        full.count_reads(reads)
    assert e.value.code == -1 and "neither sequence-only nor path-only" in str(e.value)
    # a second counter on one index, and a counter after a database load
    ix, _ = _seq_index(m, k, asm, seqs)
    ix.count_reads(reads)
    with pytest.raises(m.MfxError) as e:
        ix.count_reads(reads)
    assert e.value.code == -1 and "already took counts" in str(e.value)
    ix2, _ = _seq_index(m, k, asm, seqs)
    rk, rv = po.count_kmers(k, reads)
    ix2.add_read(rk, rv)
    with pytest.raises(m.MfxError) as e:
        ix2.count_reads(reads)
    assert e.value.code == -1 and "already took counts" in str(e.value)
    # a claim after begin
    ix3 = m.Index.for_seq(k, 10000)
    ix3.count_reads(reads)
    with pytest.raises(m.MfxError) as e:
        ix3.claim_seq(seqs)
    assert e.value.code == -1
    # a batch too small for k
    ix4, _ = _seq_index(m, k, asm, seqs)
    with pytest.raises(m.MfxError) as e:
        ix4.count_reads(reads, batch_bases=2 * k)
    assert e.value.code == -1 and "too small" in str(e.value)


def test_refusals_after_begin(tmp_path):
    """once a counter began: no database and no array on the read side; for k > 31 (every add claims there) no assembly k-mer
    either -- one claimed now would lack the reads' counts"""
    m = _mfx()
    asm, reads = sr.reads_world(21, 991, sizes=(3000,), n_reads=50)
    ix, _ = _seq_index(m, 21, asm)
    ix.count_reads(reads)
    rk, rv = po.count_kmers(21, reads)
    with pytest.raises(m.MfxError) as e:
        ix.add_read(rk, rv)
    assert e.value.code == -1 and "counted from reads" in str(e.value)
    db = str(tmp_path / "reads.txt")
    _write_text_db(db, 21, rk, rv)
    with pytest.raises(m.MfxError) as e:
        ix.load_db(db, 0)
    assert e.value.code == -1 and "counted from reads" in str(e.value)
    # k = 33: the table of the assembly's k-mers takes nothing more once its reads were counted
    k = 33
    asm, reads = sr.reads_world(k, 992, sizes=(900,), n_reads=60, lens=(40, 120))
    seqs = m.Sequences(asm)
    wx = m.Index(k, 4096)
    wx.count_asm(seqs)
    before = wx.export()
    wx.count_reads(reads)
    other = m.Sequences([sr.revcomp(asm[0])[::-1]])
    for call in (lambda: wx.count_asm(other), lambda: wx.add_asm(np.array([[5, 0]], dtype=np.uint64), np.array([1], dtype=np.uint32))):
        with pytest.raises(m.MfxError) as e:
            call()
        assert e.value.code == -1 and "give the assembly side before the reads" in str(e.value)
    with pytest.raises(m.MfxError) as e:
        wx.count_reads(reads)
    assert e.value.code == -1 and "already took counts" in str(e.value)
    after = wx.export()
    np.testing.assert_array_equal(after[0], before[0])                        # no k-mer was claimed


def test_quotient_k_mers_beyond_their_candidate_lines(monkeypatch):
    """k = 22, a table filled to 0.9: k-mers whose candidate lines are full live in the side table under their full key; the reads'
    counts reach them there (and `saturated` counts them: their read count is in the side table)"""
    m = _mfx()
    monkeypatch.setenv("MFX_LOAD_FACTOR", "0.9")
    k = 22
    asm, reads = sr.reads_world(k, 993, sizes=(60000, 20000))
    ak, av, er, rk, rv = _expected(k, asm, reads)
    assert er.max() < 2047
    seqs = m.Sequences(asm)
    ix = m.Index.for_seq(k, len(ak))
    ix.count_asm(seqs)
    info = ix.info()
    assert info["compact"] and info["distinct"] == len(ak)
    st = ix.count_reads(reads)
    ek, erv, eav = ix.export()
    np.testing.assert_array_equal(ek, ak)
    np.testing.assert_array_equal(erv, er)
    np.testing.assert_array_equal(eav, av)
    assert st["saturated"] > 0                                                 # k-mers beyond their candidate lines took read counts
    ix2 = m.Index.for_seq(k, len(ak))
    ix2.count_asm(seqs)
    ix2.add_read(rk, rv)
    for a, b in zip(ix2.export(), (ek, erv, eav)):
        np.testing.assert_array_equal(a, b)
