"""The claiming read counter (mfx_reads_begin_all, Index.count_reads_all), its table that grows (mfx_table_rehash_kernel) and the table as
a sorted database (mfx_index_write_db, Index.write_db): `meryl count` of the reads on the device.  The expected tables are the oracle's
po.count_kmers of the same records; everything is compared with ==."""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import synth, synth_reads as sr
from tests.test_gpu_parity import assert_hist_equal, oracle_hist

pytestmark = pytest.mark.gpu

START_SLOTS = 8192                                           # Index(k, 2000): the 1024-line minimum
_worlds = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _world(k, seed, **kw):
    """(asm contigs, reads, (read k-mers, counts), (asm k-mers, counts)) of a tests/synth_reads.py world, made once"""
    key = (k, seed, tuple(sorted(kw.items())))
    if key not in _worlds:
        asm, reads = sr.reads_world(k, seed, **kw)
        _worlds[key] = (asm, reads, po.count_kmers(k, reads), po.count_kmers(k, asm))
    return _worlds[key]


def _join(read, asm):
    """the table both sides give: (k-mers, read counts, assembly counts) over the union of the two oracle tables"""
    rk, rv = read
    ak, av = asm
    keys = np.union1d(rk, ak)
    r = np.zeros(len(keys), dtype=np.uint32)
    a = np.zeros(len(keys), dtype=np.uint32)
    r[np.searchsorted(keys, rk)] = rv
    a[np.searchsorted(keys, ak)] = av
    return keys, r, a


def _assert_export(ix, keys, r, a):
    ek, er, ea = ix.export()
    np.testing.assert_array_equal(ek, keys)
    np.testing.assert_array_equal(er, r)
    np.testing.assert_array_equal(ea, a)


@pytest.mark.parametrize("k", [15, 21, 22, 31])
def test_counts_equal_the_oracle_with_growth_and_without(k):
    m = _mfx()
    asm, reads, (rk, rv), _ = _world(k, 1100 + k)
    assert len(rk) > 40000                                   # 0.7 x 8 x 8192 slots = 45875: the table must reach three doublings of its start
    zeros = np.zeros(len(rk), dtype=np.uint32)
    # batches of 4096 bases: the table grows several times, each time with entries to move
    ix = m.Index(k, 2000)
    assert ix.info()["capacity"] == START_SLOTS
    st = ix.count_reads_all(reads, batch_bases=4096)
    _assert_export(ix, rk, rv, zeros)
    assert st["reads"] == len(reads) and st["bases"] == sum(len(x) for x in reads)
    assert st["kmers"] == st["counted"] == int(rv.sum()) and st["dropped"] == 0 and st["saturated"] == 0
    info, g = ix.info(), ix.growths()
    assert info["capacity"] >= 8 * START_SLOTS and info["capacity"] % START_SLOTS == 0
    assert info["distinct"] == len(rk) and info["distinct"] <= 0.7 * info["capacity"] and info["bytes"] == 16 * info["capacity"]
    assert g["growths"] >= 2 and g["rehash_bytes"] > 0
    # one batch of all reads: one growth, straight to a table that holds the batch whatever it brings
    ix1 = m.Index(k, 2000)
    ix1.count_reads_all(reads)
    _assert_export(ix1, rk, rv, zeros)
    assert ix1.growths()["growths"] == 1 and 0.35 * ix1.info()["capacity"] >= st["kmers"] and ix1.info()["capacity"] >= 8 * START_SLOTS
    # no growth: an index created with room (the batches small enough that none asks for more than the table has)
    ix2 = m.Index(k, 4 * len(rk))
    cap = ix2.info()["capacity"]
    st2 = ix2.count_reads_all(reads, batch_bases=5000)
    _assert_export(ix2, rk, rv, zeros)
    assert ix2.info()["capacity"] == cap and ix2.growths()["growths"] == 0 and st2["kmers"] == st["kmers"]


@pytest.mark.parametrize("k", [21, 31])
def test_batching_and_order_do_not_matter(k):
    m = _mfx()
    asm, reads, (rk, rv), _ = _world(k, 1200 + k, n_reads=1500)
    zeros = np.zeros(len(rk), dtype=np.uint32)
    for bb, rs in ((0, reads), (97, list(reversed(reads))), (1000, [reads[i] for i in synth.rng(3).permutation(len(reads))]), (5000, reads)):
        ix = m.Index(k, 2000)
        st = ix.count_reads_all(rs, batch_bases=bb, chunk=333)
        _assert_export(ix, rk, rv, zeros)
        assert st["kmers"] == st["counted"] == int(rv.sum()) and st["dropped"] == 0
    # the smallest batch there is, on 300 reads: the table grows between launches of a few positions
    few = reads[:300]
    fk, fv = po.count_kmers(k, few)
    ix = m.Index(k, 2000)
    st = ix.count_reads_all(few, batch_bases=2 * k + 3, chunk=50)
    _assert_export(ix, fk, fv, np.zeros(len(fk), dtype=np.uint32))
    assert st["kmers"] == int(fv.sum()) and ix.growths()["growths"] >= 2 and ix.info()["capacity"] > START_SLOTS


@pytest.mark.parametrize("k", [21, 31])
def test_contention_and_large_counts(k):
    """homopolymers, (TTAGGG)n, a 5-mer tandem array: the same few keys from every wave, claimed once, counts past 65535"""
    m = _mfx()
    _, reads, _, _ = _world(k, 1300 + k, n_reads=800)
    reads = reads + sr.low_complexity_reads(synth.rng(17), n_each=500)
    rk, rv = po.count_kmers(k, reads)
    assert rv.max() > 65535
    ix = m.Index(k, 2000)
    st = ix.count_reads_all(reads, batch_bases=5000)
    _assert_export(ix, rk, rv, np.zeros(len(rk), dtype=np.uint32))
    assert st["kmers"] == st["counted"] == int(rv.sum()) and st["dropped"] == 0


@pytest.mark.parametrize("k", [21, 22])
def test_both_sides(k):
    """the assembly counted before the reads and after them: k-mers only in the reads, only in the assembly and in both; the assembly's
    counts survive every growth, and -hist on the result is the oracle's"""
    m = _mfx()
    asm, reads, read, asmt = _world(k, 1400 + k)
    keys, r, a = _join(read, asmt)
    assert 0 < np.count_nonzero((r > 0) & (a > 0)) and np.count_nonzero(r == 0) > 0 and np.count_nonzero(a == 0) > 0
    seqs = m.Sequences(asm)
    lo, hi, peak = 3, 5000, 9.0
    _, g, ka, km = oracle_hist(k, peak, asm, read, asmt, minV=lo, maxV=hi)
    # before: a table sized for the assembly, grown by the reads with the assembly's entries in it
    before = m.Index(k, len(asmt[0]) + 16)
    before.count_asm(seqs)
    cap = before.info()["capacity"]
    before.count_reads_all(reads, batch_bases=4096, minV=lo, maxV=hi)
    assert before.growths()["growths"] >= 1 and before.info()["capacity"] > cap
    _assert_export(before, keys, r, a)
    # after: the grown table takes the assembly's claims as any full table does
    after = m.Index(k, 2000)
    after.count_reads_all(reads, batch_bases=4096, minV=lo, maxV=hi)
    after.count_asm(seqs)
    _assert_export(after, keys, r, a)
    for ix in (before, after):
        assert_hist_equal(m.Evaluator(ix, m.KParams(peak)).hist(seqs), g, ka, km, k)


def test_growth_refused():
    """-memory just above the first table: the first growth fails with MFX_E_NOMEM naming both sizes, the counter is failed, the index frees
    and the next one works"""
    m = _mfx()
    k = 21
    _, reads, (rk, rv), _ = _world(k, 1100 + k)
    L = m.load_library()

    def feed(r, recs):
        ptrs = (C.c_char_p * len(recs))(*recs)
        lens = (C.c_uint64 * len(recs))(*[len(x) for x in recs])
        return L.mfx_reads_add(r, ptrs, lens, len(recs))

    # small batches: the add that needs the larger table fails, later adds are refused, end reports the failure
    ix = m.Index(k, 2000, max_gb=0.00015)
    assert ix.info()["bytes"] == 131072
    r = L.mfx_reads_begin_all(ix.h, 1000)
    assert r
    rcs = [feed(r, reads[o:o + 100]) for o in range(0, 1000, 100)]
    first = next(i for i, rc in enumerate(rcs) if rc)
    assert rcs[first] == -2 and all(rc == 0 for rc in rcs[:first]) and all(rc == -1 for rc in rcs[first + 1:])
    from merfin_amd import binding
    st = binding._ReadsStats()
    assert L.mfx_reads_end(r, C.byref(st)) == -2
    msg = L.mfx_last_error().decode()
    assert re.search(r"cannot grow from 0\.000131 GB to 0\.000(262|524) GB", msg) and "limit of 0.000150 GB" in msg, msg
    assert ix.info()["capacity"] == START_SLOTS and ix.growths()["growths"] == 0
    ix.close()
    # one large batch: the flush of mfx_reads_end is what needs the larger table
    ix = m.Index(k, 2000, max_gb=0.00015)
    with pytest.raises(m.MfxError) as e:
        ix.count_reads_all(reads)
    assert e.value.code == -2 and "cannot grow from 0.000131 GB to" in str(e.value)
    ix.close()
    # the same limit with a table that fits it twice over: no failure; and an index without a limit afterwards
    few = reads[:60]
    fk, fv = po.count_kmers(k, few)
    assert 0.7 * START_SLOTS < len(fk) < 0.35 * 4 * START_SLOTS
    for gb in (0.0009, 0.0):
        ok = m.Index(k, 2000, max_gb=gb)
        ok.count_reads_all(few, batch_bases=1000)
        _assert_export(ok, fk, fv, np.zeros(len(fk), dtype=np.uint32))
        assert ok.growths()["growths"] == 1 and ok.info()["capacity"] == 4 * START_SLOTS


def test_refusals():
    m = _mfx()
    k = 21
    asm, reads, (rk, rv), _ = _world(k, 1100 + k)
    few = reads[:50]

    def refused(ix, text):
        with pytest.raises(m.MfxError) as e:
            ix.count_reads_all(few)
        assert e.value.code == -1 and text in str(e.value), str(e.value)

    refused(m.Index.for_seq(k, 10000), "mfx_reads_begin_all: a sequence-only or path-only index holds the k-mers claimed for it")
    refused(m.Index(33, 4096), "mfx_reads_begin_all: the table that grows holds k <= 31; this index holds 33-mers")
    sh = m.Index(k, 10000)
    sh.set_shard(0, 2)
    refused(sh, "mfx_reads_begin_all: a sharded index does not take read counts from reads")
    db = m.Index(k, len(rk) + 16)
    db.add_read(rk, rv)
    refused(db, "mfx_reads_begin_all: the read side of this index already took counts")
    _assert_export(db, rk, rv, np.zeros(len(rk), dtype=np.uint32))                     # (and it is as it was)
    twice = m.Index(k, 2000)
    twice.count_reads_all(few)
    refused(twice, "mfx_reads_begin_all: the read side of this index already took counts")
    with pytest.raises(m.MfxError) as e:
        twice.add_read(rk, rv)
    assert e.value.code == -1 and "counted from reads" in str(e.value)
    with pytest.raises(m.MfxError) as e:
        m.Index(k, 2000).count_reads_all(few, batch_bases=2 * k)
    assert e.value.code == -1 and "mfx_reads_begin_all: a batch of 42 bases is too small for 21-mers" in str(e.value)
    # the update-only counter on a full index: refused as before, with its text
    with pytest.raises(m.MfxError) as e:
        m.Index(k, 10000).count_reads(few)
    assert e.value.code == -1 and "mfx_reads_begin: the index is neither sequence-only nor path-only -- reads are counted only into k-mers claimed before" in str(e.value)


def _flat_bytes(m, tmp_path, k, kmers, values):
    p = str(tmp_path / "want.mfxk")
    m.db_write_flat(p, k, kmers, values)
    return open(p, "rb").read()


@pytest.mark.parametrize("k", [15, 21, 31])
def test_write_db(k, tmp_path, monkeypatch):
    """both sides of a table with read-only, assembly-only and shared k-mers, in one range, in ranges of about 1000 and in ranges of one
    bin: byte for byte the file mfx_db_write_flat makes of the oracle's sorted arrays"""
    m = _mfx()
    asm, reads, read, asmt = _world(k, 1500 + k, sizes=(9000, 4096, 500), n_reads=600)
    keys, r, a = _join(read, asmt)
    assert np.count_nonzero(r == 0) > 0 and np.count_nonzero(a == 0) > 0
    ix = m.Index(k, 2000)
    ix.count_reads_all(reads, batch_bases=4096)
    ix.count_asm(m.Sequences(asm))
    want = [_flat_bytes(m, tmp_path, k, *read), _flat_bytes(m, tmp_path, k, *asmt)]
    out = str(tmp_path / "got.mfxk")
    for rng in (None, "1000", "1"):
        if rng is None:
            monkeypatch.delenv("MFX_WRITE_DB_RANGE", raising=False)
        else:
            monkeypatch.setenv("MFX_WRITE_DB_RANGE", rng)
        for side in (0, 1):
            n = ix.write_db(out, side)
            assert n == len((read, asmt)[side][0])
            assert open(out, "rb").read() == want[side], (rng, side)
            assert m.db_probe(out) == {"k": k, "format": "flat", "n_kmers": n}
    _assert_export(ix, keys, r, a)                            # the table is as it was
    # the file loads as the database it is
    ix2 = m.Index(k, len(read[0]) + 16)
    ix2.load_db(str(tmp_path / "want.mfxk"), 1)                # (last written from the assembly's table)
    ix2.write_db(out, 1)
    assert open(out, "rb").read() == want[1]


def test_write_db_of_an_empty_side_and_refusals(tmp_path):
    m = _mfx()
    k = 21
    _, reads, (rk, rv), _ = _world(k, 1100 + k)
    few = reads[:40]
    ix = m.Index(k, 2000)
    ix.count_reads_all(few)
    out = str(tmp_path / "empty.mfxk")
    assert ix.write_db(out, 1) == 0
    assert open(out, "rb").read() == _flat_bytes(m, tmp_path, k, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    assert m.db_probe(out) == {"k": k, "format": "flat", "n_kmers": 0}
    assert m.Index(k, 2000).write_db(out, 0) == 0               # nothing at all in the table
    for bad, text in ((m.Index.for_seq(k, 10000), "sequence-only or path-only"), (m.Index(33, 4096), "holds k <= 31; this index holds 33-mers")):
        with pytest.raises(m.MfxError) as e:
            bad.write_db(out, 0)
        assert e.value.code == -1 and text in str(e.value)
    sh = m.Index(k, 10000)
    sh.set_shard(1, 2)
    with pytest.raises(m.MfxError) as e:
        sh.write_db(out, 0)
    assert e.value.code == -1 and "a sharded index holds part of a database only" in str(e.value)
    with pytest.raises(m.MfxError) as e:
        ix.write_db(out, 2)
    assert e.value.code == -1 and "side 2" in str(e.value)
