"""A count in passes over key ranges: the ranged claiming counter (mfx_reads_begin_range, Index.count_reads_range), the key histogram
(mfx_index_key_bins), the writer that takes several tables (mfx_db_writer_*, DbWriter) and the read store with its replay
(mfx_reads_store_*, mfx_reads_replay, ReadsStore).  The expected tables are the oracle's po.count_kmers of the same records, restricted to
the range with numpy; everything is compared with ==."""
import ctypes as C
import os

import numpy as np
import pytest

from merfin_amd import binding
from oracle import pyoracle as po
from tests import synth, synth_reads as sr

pytestmark = pytest.mark.gpu

_worlds = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _world(k, seed, low=250, **kw):
    """(asm contigs, reads, (read k-mers, counts), (asm k-mers, counts)): a tests/synth_reads.py world plus low-complexity reads, made once"""
    key = (k, seed, low, tuple(sorted(kw.items())))
    if key not in _worlds:
        asm, reads = sr.reads_world(k, seed, **kw)
        if low:
            reads = reads + sr.low_complexity_reads(synth.rng(seed + 1), n_each=low)
        _worlds[key] = (asm, reads, po.count_kmers(k, reads), po.count_kmers(k, asm))
    return _worlds[key]


def _restrict(rk, rv, lo, hi):
    sel = (rk >= np.uint64(lo)) & (rk < np.uint64(hi))
    return rk[sel], rv[sel]


def _assert_range(ix, st, rk, rv, lo, hi):
    """the table holds the oracle's k-mers of [lo, hi) with their counts, and the statistics say so"""
    wk, wv = _restrict(rk, rv, lo, hi)
    ek, er, ea = ix.export()
    np.testing.assert_array_equal(ek, wk)
    np.testing.assert_array_equal(er, wv)
    assert not ea.any()
    assert st["kmers"] == int(rv.sum(dtype=np.uint64)) and st["counted"] == int(wv.sum(dtype=np.uint64)) and st["dropped"] == 0
    return len(wk)


@pytest.mark.parametrize("k", [15, 21, 22, 31])
def test_ranged_counts_equal_the_oracle_restricted(k):
    m = _mfx()
    _, reads, (rk, rv), _ = _world(k, 2100 + k)
    top = 4 ** k
    n = len(rk)
    assert n > 40000 and rk[0] == 0 and rv[0] > 65535            # poly-A/T, counted past 16 bits
    a, b = int(rk[n // 3]), int(rk[2 * n // 3])
    tel = po.count_kmers(k, [b"TTAGGG" * 40])[0]                  # the canonical k-mers of the telomere reads: they meet in one wave and in the block table
    assert len(tel) >= 2 and np.isin(tel, rk).all()
    t1 = int(tel[1])
    thirds = [(0, a), (a, b), (b, top)]                           # a: a present k-mer as key_lo (kept) and as key_hi (left out)
    grew = 0
    counted = 0
    for lo, hi in thirds:
        ix = m.Index(k, 2000)
        st = ix.count_reads_range(reads, lo, hi, batch_bases=4096)
        assert _assert_range(ix, st, rk, rv, lo, hi) > 0
        assert st["reads"] == len(reads) and st["bases"] == sum(len(x) for x in reads)
        grew += ix.growths()["growths"]
        counted += st["counted"]
    assert grew >= 1                                              # a growth inside a ranged pass
    assert counted == int(rv.sum(dtype=np.uint64))                # over a partition, the counted k-mers are the k-mers
    others = [(0, 1), (0, t1), (t1, top), (int(rk[-1]) + 1, top), (a, a), (top, top)]
    sizes = []
    for lo, hi in others:
        ix = m.Index(k, 2000)
        st = ix.count_reads_range(reads, lo, hi, batch_bases=4096)
        sizes.append(_assert_range(ix, st, rk, rv, lo, hi))
    assert sizes[0] == 1 and sizes[1] >= 1 and sizes[1] + sizes[2] == n and sizes[3:] == [0, 0, 0]
    # [0, 4^k): count_reads_all
    full, allix = m.Index(k, 2000), m.Index(k, 2000)
    st = full.count_reads_range(reads, 0, top, batch_bases=4096)
    st_all = allix.count_reads_all(reads, batch_bases=4096)
    _assert_range(full, st, rk, rv, 0, top)
    for f in ("reads", "bases", "kmers", "counted", "dropped", "saturated"):
        assert st[f] == st_all[f]
    assert full.growths()["growths"] == allix.growths()["growths"] and full.info() == allix.info()


@pytest.mark.parametrize("k", [21, 31])
def test_ranged_batching_and_order_do_not_matter(k):
    m = _mfx()
    _, reads, (rk, rv), _ = _world(k, 2200 + k, low=60, n_reads=1500)
    top = 4 ** k
    mid = int(rk[len(rk) // 2])
    perm = [reads[i] for i in synth.rng(5).permutation(len(reads))]
    for bb, rs in ((0, reads), (97, perm), (5000, list(reversed(reads)))):
        for lo, hi in ((0, mid), (mid, top)):
            ix = m.Index(k, 2000)
            st = ix.count_reads_range(rs, lo, hi, batch_bases=bb, chunk=333)
            _assert_range(ix, st, rk, rv, lo, hi)
    # the smallest batch there is, on 300 reads
    few = reads[:300]
    fk, fv = po.count_kmers(k, few)
    mid = int(fk[len(fk) // 2])
    for lo, hi in ((0, mid), (mid, top)):
        ix = m.Index(k, 2000)
        st = ix.count_reads_range(few, lo, hi, batch_bases=2 * k + 2, chunk=50)
        _assert_range(ix, st, fk, fv, lo, hi)


def test_range_refusals():
    m = _mfx()
    k = 21
    asm, reads, (rk, rv), _ = _world(k, 2100 + k)
    few = reads[:50]
    top = 4 ** k

    def refused(ix, text, lo=0, hi=1000, **kw):
        with pytest.raises(m.MfxError) as e:
            ix.count_reads_range(few, lo, hi, **kw)
        assert e.value.code == -1 and text in str(e.value), str(e.value)

    refused(m.Index.for_seq(k, 10000), "mfx_reads_begin_range: a sequence-only or path-only index holds the k-mers claimed for it")
    refused(m.Index(33, 4096), "mfx_reads_begin_range: the table that grows holds k <= 31; this index holds 33-mers")
    sh = m.Index(k, 10000)
    sh.set_shard(0, 2)
    refused(sh, "mfx_reads_begin_range: a sharded index does not take read counts from reads")
    db = m.Index(k, len(rk) + 16)
    db.add_read(rk, rv)
    refused(db, "mfx_reads_begin_range: the read side of this index already took counts")
    refused(m.Index(k, 2000), "mfx_reads_begin_range: a batch of 42 bases is too small for 21-mers", batch_bases=2 * k)
    fresh = m.Index(k, 2000)
    refused(fresh, "mfx_reads_begin_range: the range starts above its end (key_lo 8 > key_hi 7)", lo=8, hi=7)
    refused(fresh, "mfx_reads_begin_range: the range ends beyond the 21-mers (key_hi %d > 4^21 = %d)" % (top + 1, top), lo=0, hi=top + 1)
    # a refused range leaves the index as it was: it takes the counter afterwards
    st = fresh.count_reads_range(few, 0, top)
    assert st["counted"] == st["kmers"] > 0
    refused(fresh, "mfx_reads_begin_range: the read side of this index already took counts")


def _bincount(k, keys):
    bits = min(2 * k, 12)
    return np.bincount((keys >> np.uint64(2 * k - bits)).astype(np.int64), minlength=1 << bits).astype(np.uint64)


@pytest.mark.parametrize("k", [5, 15, 21, 31])
def test_key_bins(k):
    m = _mfx()
    asm, reads, (rk, rv), (ak, av) = _world(k, 2300 + k, low=0, sizes=(9000, 4096, 500), n_reads=600)
    ix = m.Index(k, 2000)
    ix.count_reads_all(reads, batch_bases=4096)
    ix.count_asm(m.Sequences(asm))
    for side, keys in ((0, rk), (1, ak)):
        bins = ix.key_bins(side)
        assert bins.dtype == np.uint64 and len(bins) == 1 << min(2 * k, 12)
        np.testing.assert_array_equal(bins, _bincount(k, keys))
    with pytest.raises(m.MfxError) as e:
        ix.key_bins(2)
    assert e.value.code == -1 and "mfx_index_key_bins: side 2" in str(e.value)
    with pytest.raises(m.MfxError) as e:
        m.Index.for_seq(k, 10000).key_bins()
    assert e.value.code == -1 and "mfx_index_key_bins: a sequence-only or path-only index" in str(e.value)


def test_key_bins_after_a_refused_growth():
    """the counter fails with MFX_E_NOMEM under max_gb: the index can still be read, and its bins are those of its own export"""
    m = _mfx()
    k = 21
    _, reads, (rk, rv), _ = _world(k, 2100 + k)
    for begin in (lambda ix: ix.count_reads_all(reads, batch_bases=1000), lambda ix: ix.count_reads_range(reads, 0, int(rk[len(rk) // 2]), batch_bases=1000)):
        ix = m.Index(k, 2000, max_gb=0.00015)
        with pytest.raises(m.MfxError) as e:
            begin(ix)
        assert e.value.code == -2 and "cannot grow from 0.000131 GB to" in str(e.value)
        info = ix.info()
        assert info["bytes"] == 131072 and 0 < info["distinct"] <= 0.7 * info["capacity"]
        ek, er, _ = ix.export()
        assert len(ek) == info["distinct"] and er.all() and np.isin(ek, rk).all()
        np.testing.assert_array_equal(ix.key_bins(0), _bincount(k, ek))
        ix.close()


def _flat_bytes(m, tmp_path, k, kmers, values):
    p = str(tmp_path / "want.mfxk")
    m.db_write_flat(p, k, kmers, values)
    return open(p, "rb").read()


@pytest.mark.parametrize("k", [15, 21, 31])
def test_writer_of_several_tables(k, tmp_path, monkeypatch):
    m = _mfx()
    _, reads, (rk, rv), _ = _world(k, 2400 + k, low=0, sizes=(9000, 4096, 500), n_reads=600)
    top = 4 ** k
    n = len(rk)
    a, b = int(rk[n // 3]), int(rk[2 * n // 3])
    want = _flat_bytes(m, tmp_path, k, rk, rv)
    one = m.Index(k, 2000)
    one.count_reads_all(reads, batch_bases=4096)
    out = str(tmp_path / "one.mfxk")
    assert one.write_db(out) == n and open(out, "rb").read() == want
    parts = []
    for lo, hi in ((0, a), (a, b), (b, top)):
        ix = m.Index(k, 2000)
        ix.count_reads_range(reads, lo, hi, batch_bases=4096)
        parts.append(ix)
    empty = m.Index(k, 2000)
    out = str(tmp_path / "passes.mfxk")
    for rng in (None, "1000"):
        if rng is None:
            monkeypatch.delenv("MFX_WRITE_DB_RANGE", raising=False)
        else:
            monkeypatch.setenv("MFX_WRITE_DB_RANGE", rng)
        if os.path.exists(out):
            os.remove(out)
        w = m.DbWriter(out, k)
        added = [w.append(parts[0]), w.append(empty), w.append(parts[1])]             # an empty append in the middle changes nothing
        assert added == [n // 3, 0, 2 * n // 3 - n // 3]
        for late in (parts[0], parts[1]):                                              # out of order: refused, nothing added
            with pytest.raises(m.MfxError) as e:
                w.append(late)
            assert e.value.code == -1 and "not above the writer's last k-mer %d" % int(rk[2 * n // 3 - 1]) in str(e.value), str(e.value)
        assert w.append(parts[2]) == n - 2 * n // 3
        assert not os.path.exists(out)                                                # nothing exists before close
        assert w.close() == n
        assert open(out, "rb").read() == want, rng
        assert m.db_probe(out) == {"k": k, "format": "flat", "n_kmers": n}
    monkeypatch.delenv("MFX_WRITE_DB_RANGE", raising=False)
    # abort leaves no file; a close of nothing is write_db of an empty side
    gone = str(tmp_path / "gone.mfxk")
    w = m.DbWriter(gone, k)
    assert w.append(parts[1]) > 0
    w.abort()
    assert not os.path.exists(gone)
    w = m.DbWriter(gone, k)
    assert w.close() == 0
    nothing = str(tmp_path / "nothing.mfxk")
    assert one.write_db(nothing, 1) == 0
    assert open(gone, "rb").read() == open(nothing, "rb").read()
    # another k, a side that does not exist: refused, the writer as it was
    w = m.DbWriter(gone, k)
    with pytest.raises(m.MfxError) as e:
        w.append(m.Index(k + 1 if k < 31 else 30, 2000))
    assert e.value.code == -1 and "mfx_db_writer_append_index: the writer holds %d-mers" % k in str(e.value)
    with pytest.raises(m.MfxError) as e:
        w.append(parts[0], side=2)
    assert e.value.code == -1 and "mfx_db_writer_append_index: side 2" in str(e.value)
    w.abort()


def test_store_and_replay():
    m = _mfx()
    k = 21
    asm, reads, (rk, rv), (ak, av) = _world(k, 2500 + k, low=60, n_reads=1500)
    top = 4 ** k
    mid = int(rk[len(rk) // 2])
    n_bases = sum(len(x) for x in reads)
    stores = []
    for chunk in (1, 97, len(reads)):
        s = m.ReadsStore(k, 4096)
        assert s.add(reads, chunk=chunk)
        info = s.info()
        assert info["reads"] == len(reads) and info["bases"] == n_bases and info["complete"] and info["batches"] > 50
        stores.append(s)
        for lo, hi in ((0, top), (mid, top)):
            ix = m.Index(k, 2000)
            st = s.replay(ix, key_range=(lo, hi), batch_bases=4096)
            _assert_range(ix, st, rk, rv, lo, hi)
            assert st["reads"] == len(reads) and st["bases"] == n_bases
            assert ix.growths()["growths"] >= 1                    # the growth bound holds per replayed batch
    assert stores[0].info() == stores[1].info() == stores[2].info()
    s = stores[0]
    full = s.info()
    # batch by batch, and through a counter with larger batches: the same table
    ix = m.Index(k, 2000)
    L = m.load_library()
    r = L.mfx_reads_begin_range(ix.h, 10000, 0, mid)
    assert r
    for i in range(full["batches"]):
        assert L.mfx_reads_replay(r, s.h, i, 1) == 0
    assert L.mfx_reads_replay(r, s.h, full["batches"], 1) == -1 and "of a store of %d" % full["batches"] in L.mfx_last_error().decode()
    st = binding._ReadsStats()
    assert L.mfx_reads_end(r, C.byref(st)) == 0                   # (a refused replay sends nothing and fails nothing)
    _assert_range(ix, {f: getattr(st, f) for f, _ in binding._ReadsStats._fields_}, rk, rv, 0, mid)
    assert st.reads == len(reads) and st.bases == n_bases


def test_store_refusals_and_the_update_only_counter():
    m = _mfx()
    k = 21
    asm, reads, (rk, rv), (ak, av) = _world(k, 2500 + k, low=60, n_reads=1500)
    s = m.ReadsStore(k, 4096)
    assert s.add(reads)
    full = s.info()
    # one batch short: add says so, the store is incomplete, replay refuses it
    short = m.ReadsStore(k, 4096, max_bytes=full["bytes"] - 12)
    assert short.add(reads, chunk=97) is False and short.add(reads[:1]) is False
    assert short.info()["complete"] is False
    with pytest.raises(m.MfxError) as e:
        short.replay(m.Index(k, 2000))
    assert e.value.code == -1 and "mfx_reads_replay: the store is incomplete" in str(e.value)
    exact = m.ReadsStore(k, 4096, max_bytes=full["bytes"])
    assert exact.add(reads, chunk=97) and exact.info() == full
    with pytest.raises(m.MfxError) as e:
        s.replay(m.Index(22, 2000))
    assert e.value.code == -1 and "mfx_reads_replay: the store holds batches cut for 21-mers, the counter counts 22-mers" in str(e.value)
    with pytest.raises(m.MfxError) as e:
        s.replay(m.Index(k, 2000), batch_bases=4095)
    assert e.value.code == -1 and "mfx_reads_replay: the counter's batch of 4095 bases is smaller than the store's of 4096" in str(e.value)
    with pytest.raises(m.MfxError) as e:
        m.ReadsStore(k, 2 * k)
    assert e.value.code == -1 and "mfx_reads_store_create: a batch of 42 bases is too small for 21-mers" in str(e.value)
    # the update-only counter of a sequence-only index: replay is count_reads
    seqs = m.Sequences(asm)
    got = []
    for how in ("replay", "count_reads"):
        ix = m.Index.for_seq(k, sum(len(c) for c in asm) + 16)
        ix.count_asm(seqs)
        st = s.replay(ix, update_only=True, batch_bases=5000) if how == "replay" else ix.count_reads(reads, batch_bases=4096)
        got.append((ix.export(), {f: st[f] for f in ("reads", "bases", "kmers", "counted", "dropped", "saturated")}))
    for x, y in zip(got[0][0], got[1][0]):
        np.testing.assert_array_equal(x, y)
    assert got[0][1] == got[1][1] and got[0][1]["counted"] > 0 and got[0][1]["dropped"] > 0
