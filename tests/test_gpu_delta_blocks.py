"""The two kernels that decode a delta-coded database into the table (mfx_table_add_delta_kernel for k-mer-sorted files,
mfx_table_add_placed_kernel for placed ones), block by block: the catalogue of tests/delta_blocks.py -- field widths from 0 to the
record's own and wider than the narrowest, every escape boundary, the last-block lengths at which the lanes, waves and rounds split,
one large difference at each seam, several blocks per workgroup (MFX_INGEST_GRID), several launches per load -- into the full
table, the sequence-only table of 16-byte slots, the compact layout's direct and quotient form and three shards, on both sides.
After every load export() equals a plain dict, with == and no tolerance anywhere."""
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import delta_blocks as db
from tests.test_placed_db import canon

pytestmark = pytest.mark.gpu


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def catalogues():
    return {}


def _cases(catalogues, k):
    if k not in catalogues:
        catalogues[k] = db.synthetic(k)
    return catalogues[k]


def _all_canonical(k, c):
    x = np.array([a for a, v in zip(c.kmers, c.counts) if v], dtype=np.uint64)
    y, rc = x.copy(), np.zeros_like(x)
    for _ in range(k):                                             # complement of a 2-bit code: code ^ 2
        rc = (rc << np.uint64(2)) | ((y & np.uint64(3)) ^ np.uint64(2))
        y >>= np.uint64(2)
    return bool((x <= rc).all())


def _arrays(table):
    keys = np.array(sorted(table), dtype=np.uint64)
    return keys, np.array([table[x] for x in keys.tolist()], dtype=np.uint32)


def _check_full(ix, table, side, what):
    keys, vals = _arrays(table)
    ek, er, ea = ix.export()
    np.testing.assert_array_equal(ek, keys, err_msg=what)
    np.testing.assert_array_equal(ea if side else er, vals, err_msg=what)
    assert not (er if side else ea).any(), what
    info = ix.info()
    assert info["distinct"] == len(keys) and info["dropped"] == 0, what


def _check_shards(m, k, path, n, table, side, what):
    """three shards of a full table, loaded together: each takes its own k-mers, and together they hold the dict"""
    shards = [m.Index(k, n + 16) for _ in range(3)]
    for r, s in enumerate(shards):
        s.set_shard(r, 3)
    m.load_db_multi(shards, path, side)
    got = [s.export() for s in shards]
    ek = np.concatenate([g[0] for g in got])
    ev = np.concatenate([g[2 if side else 1] for g in got])
    o = np.argsort(ek)
    keys, vals = _arrays(table)
    np.testing.assert_array_equal(ek[o], keys, err_msg=what)
    np.testing.assert_array_equal(ev[o], vals, err_msg=what)
    assert not np.concatenate([g[1 if side else 2] for g in got]).any(), what
    assert sum(s.info()["distinct"] for s in shards) == len(keys), what
    assert len(keys) < 64 or all(len(g[0]) for g in got), what


@pytest.mark.parametrize("k", [15, 21, 31])
def test_full_table_takes_the_catalogue(k, catalogues, tmp_path, monkeypatch):
    m = _mfx()
    for c in _cases(catalogues, k):
        path = c.write(str(tmp_path / (c.name + ".mfxk")))
        table, _ = db.expected(c.kmers, c.counts)
        for side in (0, 1):
            ix = m.Index(k, len(c.kmers) + 16)
            ix.load_db(path, side)
            _check_full(ix, table, side, "%s side %d" % (c.name, side))
            assert ix.info()["canonical"] == _all_canonical(k, c)   # (the full table takes any k-mer and says whether it saw a non-canonical one)
        # one workgroup takes every block of the file in turn
        monkeypatch.setenv("MFX_INGEST_GRID", "1")
        ix = m.Index(k, len(c.kmers) + 16)
        ix.load_db(path, 0)
        monkeypatch.delenv("MFX_INGEST_GRID")
        _check_full(ix, table, 0, c.name + " grid 1")
        for side in (0, 1):
            _check_shards(m, k, path, len(c.kmers), table, side, c.name)
        if c.name == "widths":
            # -min / -max around the escape boundary of the 11-bit block and of the 21-bit one: applied to the resolved count
            lo, hi = (1 << 11) - 1, (1 << 21) - 2
            ix = m.Index(k, len(c.kmers) + 16)
            ix.load_db(path, 0, lo, hi)
            q = np.array(c.kmers, dtype=np.uint64)
            rv, av = ix.value(q)
            want = np.array([v if lo <= v <= hi else 0 for v in c.counts], dtype=np.uint32)
            np.testing.assert_array_equal(rv, want)
            assert {lo - 1, lo, hi, hi + 1} <= set(c.counts) and not av.any()


@pytest.mark.parametrize("k", [15, 21, 31])
def test_several_blocks_per_workgroup(k, catalogues, tmp_path, monkeypatch):
    """ten blocks of alternating widths, first k-mers far apart, by 1, 2, 3 and 4 workgroups and by one workgroup per block: the state a
    workgroup carries from block to block (wsum, s_base) behind its barrier"""
    m = _mfx()
    c = next(x for x in _cases(catalogues, k) if x.name == "grid")
    path = c.write(str(tmp_path / "grid.mfxk"))
    table, _ = db.expected(c.kmers, c.counts)
    for grid in ("1", "2", "3", "4", None, "0", "8193"):          # (outside 1..8192: the default)
        if grid is None:
            monkeypatch.delenv("MFX_INGEST_GRID", raising=False)
        else:
            monkeypatch.setenv("MFX_INGEST_GRID", grid)
        for side in (0, 1):
            ix = m.Index(k, len(c.kmers) + 16)
            ix.load_db(path, side)
            _check_full(ix, table, side, "grid %s side %d" % (grid, side))


@pytest.mark.parametrize("k", [15, 21, 31])
def test_a_load_cut_into_several_launches(k, tmp_path, monkeypatch, capfd):
    """1.3 MB of wide blocks through the smallest staging lanes: more than one launch (payload_base > 0 from the second on), counted
    from the loader's own report; the same table by one launch, by a staged load, and with several blocks per workgroup"""
    m = _mfx()
    c, nbytes = db.launches_case(k)
    path = c.write(str(tmp_path / "l.mfxk"))
    table, _ = db.expected(c.kmers, c.counts)
    # the loader reports every ingest it makes, the blocks' and the escape list's alike: the escape list (fewer entries than the smallest lane
    # holds) is one chunk always, so a report of three chunks or more is the blocks'
    assert sum(v >= (1 << 22) - 1 for v in c.counts) < 1 << 16
    report = re.compile(r"-- ingest: .*?(\d+) chunks")
    monkeypatch.setenv("MFX_INGEST_TIMING", "1")
    capfd.readouterr()
    ix = m.Index(k, len(c.kmers) + 16)
    ix.load_db(path, 0)
    chunks = [int(x) for x in report.findall(capfd.readouterr().err)]
    assert chunks and set(chunks) == {1}, chunks                  # by default: one launch
    _check_full(ix, table, 0, "one launch")
    monkeypatch.setenv("MFX_INGEST_CHUNK_LOG2", "16")
    for grid in (None, "3"):
        if grid:
            monkeypatch.setenv("MFX_INGEST_GRID", grid)
        capfd.readouterr()
        ix = m.Index(k, len(c.kmers) + 16)
        ix.load_db(path, 1)
        err = capfd.readouterr().err
        chunks = [int(x) for x in report.findall(err)]
        assert chunks and max(chunks) >= 3, err                    # 512 KB lanes: the blocks' 1.3 MB take three chunks or more
        _check_full(ix, table, 1, "several launches, grid %s" % grid)
    monkeypatch.delenv("MFX_INGEST_GRID")
    monkeypatch.delenv("MFX_INGEST_CHUNK_LOG2")
    monkeypatch.delenv("MFX_INGEST_TIMING")
    st = m.DbStage(path)
    assert st.ok, st.why
    ix = m.Index(k, len(c.kmers) + 16)
    ix.load_db_staged(st, 0)
    st.close()
    _check_full(ix, table, 0, "staged")


# ---- the tables with a frozen key set: the canonical k-mers of a sequence, plus foreign ones that are dropped ----
def _counts_by_position(k, n, rng, placed31):
    """counts by the record's place in the file: block b holds the counts of vbits class b mod 6 (k = 31 placed: the field holds
    count << 1 | strand bit, so a class of vbits takes counts of vbits - 1)"""
    out = []
    for b in range((n + db.BLOCK - 1) // db.BLOCK):
        vb = db.VBIT_CLASSES[b % 6] - (1 if placed31 and db.VBIT_CLASSES[b % 6] > 2 else 0)
        cnt = db._counts_for(vb, min(db.BLOCK, n - b * db.BLOCK), rng, every_escape=(b == 7))
        if b % 6 == 5 and len(cnt) > 300:
            # the fold of a placed 31-mer file: the last two escape there.  At places 3 mod 32, where worlds() keeps a count of 2047 or more
            cnt[99], cnt[195], cnt[291] = (1 << 20) - 1, (1 << 21) - 1, 1 << 21
        out += cnt
    return out


def _placed_order(m, k, keys, tmp):
    """the k-mers in the order of a placed file's records.  k <= 30: by their placement numbers; k = 31 (65 bits, made inside the
    converter only): a placed file whose every count escapes lists its k-mers, in the file's order, as its escape list"""
    if k <= 30:
        return keys[np.argsort(m.db_place_keys(k, keys), kind="stable")]
    m.db_write_flat(tmp + ".f", k, keys, np.full(len(keys), 1 << 31, dtype=np.uint32))
    assert m.db_convert_placed(tmp + ".f", tmp + ".p") == len(keys)
    raw = db.decode_raw(tmp + ".p")
    assert len(raw.escapes) == len(keys)
    return np.array([e[0] for e in raw.escapes], dtype=np.uint64)


def _forced(rec_bits):
    def f(b, kb, vb):
        return [(kb, vb), (rec_bits, db.MAX_VBITS), (min(kb + 1, rec_bits), min(vb + 1, db.MAX_VBITS)), (max(kb, min(33, rec_bits)), vb),
                (kb, db.MAX_VBITS), (max(kb, min(32, rec_bits)), max(vb, 12))][(b + b // 6) % 6]
    return f


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    made = {}

    def get(k):
        if k in made:
            return made[k]
        m = _mfx()
        d = tmp_path_factory.mktemp("w%d" % k)
        rng = np.random.default_rng(5000 + k)
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 150000)].tobytes()
        ak, av = po.count_kmers(k, [seq])
        # k-mers whose placement numbers lie 1 and 2 apart (the placed kernel's narrowest fields); k = 15 has no placed catalogue
        tw = db.twins(k, rng, 2) if k >= 21 else []
        extra = [x for pair in tw + (db.window_neighbours(k, rng, 2) if k >= 21 else []) for x in pair]
        planted = set(extra)
        foreign = np.setdiff1d(np.unique(np.concatenate([canon(rng, k, len(ak) // 20), np.array(extra, dtype=np.uint64)])), ak)
        keys = np.union1d(ak, foreign)
        claimed = set(ak.tolist())
        w = {"k": k, "seq": seq, "ak": ak, "av": av, "sets": []}
        for shape in ("sorted", "placed"):
            order = keys if shape == "sorted" else _placed_order(m, k, keys, str(d / "order"))
            if shape == "placed" and k == 31:
                # the twins (equal stored numbers, strand bit 0 then 1): the first pair's records in two rounds (entries 1023 | 1024 of a block), the
                # second pair's in two lanes (entries 4j + 3 | 4j + 4) -- by leaving out records that come before them
                ol = order.tolist()
                (a1, b1), (a2, b2) = sorted(tw, key=lambda t: ol.index(t[0]))
                i1 = ol.index(a1)
                assert ol[i1 + 1] == b1 and i1 > 1024
                del ol[:(i1 - 1023) % 1024]
                i1, i2 = ol.index(a1), ol.index(a2)
                assert i1 % 1024 == 1023 and ol[i2 + 1] == b2 and i2 - i1 > 8
                del ol[i1 + 2:i1 + 2 + (i2 - 3) % 4]
                i2 = ol.index(a2)
                assert i2 % 4 == 3 and i2 % 1024 != 1023 and ol.index(a1) % 1024 == 1023
                order = np.array(ol, dtype=np.uint64)
                w["twins"] = ((a1, b1), (a2, b2))
            counts = _counts_by_position(k, len(order), rng, shape == "placed" and k == 31)
            # the sequence's own k-mers: one count in thirty-two of those that saturate a compact slot's 11-bit field stays (the side table that holds
            # their exact counts is sized for rare ones), none wraps 32 bits when side 1 adds it to the sequence's count; the foreign ones keep theirs
            counts = [c if x not in claimed else min(c, 4000000000) if c < 2047 or i % 32 == 3 else c % 2000
                      for i, (x, c) in enumerate(zip(order.tolist(), counts))]
            counts = [c or 1 if x in planted else c for x, c in zip(order.tolist(), counts)]      # (the planted pairs are stored: no zero count)
            o = np.argsort(order)
            skeys, svals = order[o], np.array(counts, dtype=np.uint32)[o]
            flat, placed = str(d / (shape + ".flat")), str(d / (shape + ".placed"))
            m.db_write_flat(flat, k, skeys, svals)
            assert m.db_convert_placed(flat, placed) == len(skeys)
            src = flat if shape == "sorted" else placed
            forced = src + ".forced"
            rec_bits = 2 * k if shape == "sorted" else 64 if k == 31 else max(2 * k + 3, 41)
            raw = db.reencode(src, forced, _forced(rec_bits))
            again = db.decode_raw(forced)
            assert again.records == raw.records and again.fields == raw.fields and again.widths != raw.widths
            table, dropped = db.expected(skeys.tolist(), svals.tolist(), claimed)
            full, _ = db.expected(skeys.tolist(), svals.tolist())
            w["sets"].append({"shape": shape, "files": {"flat": flat, "placed": placed, "forced": forced}, "table": table, "dropped": dropped,
                              "full": full, "n": len(skeys), "widths": again.widths, "lib_widths": raw.widths, "records": raw.records,
                              "raw": raw, "order": order.tolist(), "counts": counts})
        made[k] = w
        return w
    return get


def _check_frozen(ix, w, s, side, what):
    ek, er, ea = ix.export()
    np.testing.assert_array_equal(ek, w["ak"], err_msg=what)
    add = np.array([s["table"].get(x, 0) for x in w["ak"].tolist()], dtype=np.uint32)
    np.testing.assert_array_equal(er, add if side == 0 else np.zeros_like(add), err_msg=what)
    np.testing.assert_array_equal(ea, (w["av"] + add).astype(np.uint32) if side == 1 else w["av"], err_msg=what)
    info = ix.info()
    assert info["distinct"] == len(w["ak"]) and info["dropped"] == s["dropped"] and s["dropped"] > 0, what


@pytest.mark.parametrize("k,compact", [(21, "0"), (31, "0"), (15, "1"), (21, "1"), (22, "1"), (31, "1")])
def test_frozen_tables_take_sorted_and_placed_files_at_forced_widths(k, compact, worlds, monkeypatch):
    """16-byte slots (compact 0), the compact layout's direct form (k <= 21) and its quotient form: the records of a sequence's k-mers and
    5 % foreign ones, as the library's sorted and placed file and written again at other widths, sides 0 and 1; the placed file with
    (compact) and without (16-byte slots) the table taking the records' own placement"""
    m = _mfx()
    w = worlds(k)
    seqs = m.Sequences([w["seq"]])

    def load(path, side, env=()):
        monkeypatch.setenv("MFX_SEQ_COMPACT", compact)
        ix = m.Index.for_seq(k, len(w["seq"]) + 16)
        monkeypatch.delenv("MFX_SEQ_COMPACT")
        assert ix.info()["compact"] == (compact == "1")
        ix.count_asm(seqs)
        for name, v in env:
            monkeypatch.setenv(name, v)
        ix.load_db(path, side)
        for name, v in env:
            monkeypatch.delenv(name)
        return ix
    for s in w["sets"]:
        for name, path in s["files"].items():
            for side in (0, 1):
                _check_frozen(load(path, side), w, s, side, "%s/%s side %d" % (s["shape"], name, side))
        for env in ((("MFX_INGEST_GRID", "1"),), (("MFX_INGEST_GRID", "3"),), (("MFX_INGEST_CHUNK_LOG2", "16"),)):
            _check_frozen(load(s["files"]["forced"], 0, env), w, s, 0, "%s/forced %s" % (s["shape"], env))
    # -min / -max: applied to the resolved count, escaped or not
    s = w["sets"][1]
    lo, hi = 3, (1 << 21) - 1
    monkeypatch.setenv("MFX_SEQ_COMPACT", compact)
    ix = m.Index.for_seq(k, len(w["seq"]) + 16)
    monkeypatch.delenv("MFX_SEQ_COMPACT")
    ix.count_asm(seqs)
    ix.load_db(s["files"]["forced"], 0, lo, hi)
    rv, av = ix.value(w["ak"])
    want = np.array([s["table"].get(x, 0) for x in w["ak"].tolist()], dtype=np.uint64)
    np.testing.assert_array_equal(rv, np.where((want >= lo) & (want <= hi), want, 0).astype(np.uint32))
    np.testing.assert_array_equal(av, w["av"])
    assert ((want > 0) & (want < lo)).any() and (want == hi).any() and (want == hi + 1).any()


@pytest.mark.parametrize("k", [21, 30, 31])
def test_full_table_takes_the_placed_files(k, worlds):
    """... and the full table, which places every record anew and keeps the foreign k-mers: what shows a wrong decode of a record that a
    frozen table would only drop.  k = 30: stored numbers of 63 bits; k = 31: of 64, twins across a round's and a lane's seam"""
    m = _mfx()
    w = worlds(k)
    for s in w["sets"]:
        for name in ("placed", "forced"):
            for side in (0, 1):
                ix = m.Index(k, s["n"] + 16)
                ix.load_db(s["files"][name], side)
                _check_full(ix, s["full"], side, "%s/%s side %d" % (s["shape"], name, side))
    s = w["sets"][1]
    rec = s["records"]
    kbits = {kb for kb, vb in s["widths"]}
    assert (64 if k == 31 else 2 * k + 3) in kbits and {vb for kb, vb in s["widths"]} >= {3, 12, 22}
    # a block whose running sum crosses 2^62 (the numbers of k >= 30 fill their 63 / 64 bits)
    if k >= 30:
        assert any(rec[b] < 1 << 62 <= rec[min(b + db.BLOCK, len(rec)) - 1] for b in range(0, len(rec), db.BLOCK))
    if k == 31:
        i = [j for j in range(len(rec) - 1) if rec[j] == rec[j + 1]]
        ol = {rec[j] for j in i}
        assert any(j % 1024 == 1023 for j in i) and any(j % 4 == 3 and j % 1024 != 1023 for j in i) and len(ol) == len(i)
        assert all(s["full"][x] > 0 for pair in w["twins"] for x in pair)


@pytest.mark.parametrize("k", [21, 22])
def test_placed_update_plain_store_boundary(k, worlds, tmp_path, monkeypatch):
    """the placed update writes a slot's word with a plain store while field + count stays below the field's saturation value (2047), and
    goes through the compare-and-swap path -- the exact count moves to the side table -- from there on: fields preset to 0, 1, 2045, 2046,
    2047 (and far beyond), the file adds 1, 2, 2046, 2047, on both sides; every sum below, at and above 2047"""
    m = _mfx()
    w = worlds(k)
    seqs = m.Sequences([w["seq"]])
    ak = w["ak"]
    presets, adds = (0, 1, 2045, 2046, 2047, 70000), (1, 2, 2046, 2047)
    rng = np.random.default_rng(77 + k)
    pick = rng.choice(len(ak), 24 * 16, replace=False).reshape(24, 16)
    pre, add = {}, {}
    for g, (p, a) in enumerate((p, a) for p in presets for a in adds):
        for i in pick[g]:
            pre[int(ak[i])], add[int(ak[i])] = p, a
    assert {p + a for p in presets for a in adds} >= {2046, 2047, 2048}
    fk = np.array(sorted(add), dtype=np.uint64)
    fv = np.array([add[x] for x in fk.tolist()], dtype=np.uint32)
    flat, placed = str(tmp_path / "b.flat"), str(tmp_path / "b.placed")
    m.db_write_flat(flat, k, fk, fv)
    assert m.db_convert_placed(flat, placed) == len(fk)
    pk = np.array([x for x in sorted(pre) if pre[x]], dtype=np.uint64)
    pv = np.array([pre[x] for x in pk.tolist()], dtype=np.uint32)
    for compact in ("1", "0"):
        for side in (0, 1):
            for path in (placed, flat):
                monkeypatch.setenv("MFX_SEQ_COMPACT", compact)
                ix = m.Index.for_seq(k, len(w["seq"]) + 16)
                monkeypatch.delenv("MFX_SEQ_COMPACT")
                if side == 0:
                    ix.count_asm(seqs)
                    ix.add_read(pk, pv)
                else:
                    ix.claim_seq(seqs)
                    ix.add_asm(pk, pv)
                _, r0, a0 = ix.export()
                base = np.array([pre.get(x, 0) for x in ak.tolist()], dtype=np.uint32)
                np.testing.assert_array_equal(a0 if side else r0, base)
                ix.load_db(path, side)
                ek, er, ea = ix.export()
                np.testing.assert_array_equal(ek, ak)
                want = base + np.array([add.get(x, 0) for x in ak.tolist()], dtype=np.uint32)
                np.testing.assert_array_equal(ea if side else er, want, err_msg="compact %s side %d %s" % (compact, side, path))
                np.testing.assert_array_equal(er if side else ea, np.zeros_like(want) if side else w["av"])
                assert ix.info()["dropped"] == 0


@pytest.mark.parametrize("k", [21, 22, 30, 31])
def test_placed_kernel_takes_its_catalogue(k, worlds, tmp_path, monkeypatch):
    """mfx_table_add_placed_kernel at the blocks where it splits: the world's placed file (the library's own placement numbers) cut to every
    last-block length, one record, two-record last blocks of the narrowest fields (twins, window neighbours), one jump of 2^40 or more
    among consecutive records at each seam of its lanes, waves and rounds of 1024, ten blocks of alternating widths by 1 .. 4 workgroups
    -- into the full table (every record placed anew), three shards, and the frozen tables with and without the records' own placement"""
    m = _mfx()
    w = worlds(k)
    s = w["sets"][1]
    src = s["raw"]
    src.kmers, claimed = s["order"], set(w["ak"].tolist())
    seqs = m.Sequences([w["seq"]])
    big = db.placed_big(k)
    assert big >= 1 << 40
    for name, idx, widths in db.placed_cuts(k, src.records, src.kmers, big):
        path = db.write_cut(str(tmp_path / (name + ".mfxk")), src, idx, widths)
        assert m.db_probe(path).get("placed")
        kmers, counts = [src.kmers[i] for i in idx], [s["counts"][i] for i in idx]
        full, _ = db.expected(kmers, counts)
        for grid in (None, "1") + (("2", "3", "4") if name == "grid" else ()):
            if grid:
                monkeypatch.setenv("MFX_INGEST_GRID", grid)
            for side in (0, 1):
                ix = m.Index(k, len(idx) + 16)
                ix.load_db(path, side)
                _check_full(ix, full, side, "%s grid %s side %d" % (name, grid, side))
            if grid:
                monkeypatch.delenv("MFX_INGEST_GRID")
        _check_shards(m, k, path, len(idx), full, 0, name)
        table, dropped = db.expected(kmers, counts, claimed)
        add = np.array([table.get(x, 0) for x in w["ak"].tolist()], dtype=np.uint32)
        for compact in ("1", "0") if k != 30 else ():
            for side in (0, 1):
                monkeypatch.setenv("MFX_SEQ_COMPACT", compact)
                ix = m.Index.for_seq(k, len(w["seq"]) + 16)
                monkeypatch.delenv("MFX_SEQ_COMPACT")
                ix.count_asm(seqs)
                ix.load_db(path, side)
                ek, er, ea = ix.export()
                what = "%s compact %s side %d" % (name, compact, side)
                np.testing.assert_array_equal(ek, w["ak"], err_msg=what)
                np.testing.assert_array_equal(er, add if side == 0 else np.zeros_like(add), err_msg=what)
                np.testing.assert_array_equal(ea, (w["av"] + add).astype(np.uint32) if side == 1 else w["av"], err_msg=what)
                assert ix.info()["dropped"] == dropped, what


def test_a_real_64_bit_difference_on_the_device(tmp_path):
    """the placed 31-mer files of two or three k-mers whose neighbouring records lie 2^63 or more apart (the files of
    tests/test_delta_blocks_cpu.py): kbits = 64 with a difference that needs the field's top bit, into the full table"""
    m = _mfx()
    k, found = 31, 0
    for seed in range(64):
        r = np.random.default_rng(7000 + seed)
        km = canon(r, k, 2 + seed % 2)
        if len(km) < 2:
            continue
        vals = np.array([5, (1 << 21) + 1, 70000][:len(km)], dtype=np.uint32)
        flat, placed = str(tmp_path / "f.mfxk"), str(tmp_path / "p.mfxk")
        m.db_write_flat(flat, k, km, vals)
        assert m.db_convert_placed(flat, placed) == len(km)
        raw = db.decode_raw(placed)
        if max(y - x for x, y in zip(raw.records, raw.records[1:])) < 1 << 63:
            continue
        found += 1
        assert raw.widths[0][0] == 64
        for side in (0, 1):
            ix = m.Index(k, 64)
            ix.load_db(placed, side)
            _check_full(ix, dict(zip(km.tolist(), vals.tolist())), side, "seed %d side %d" % (seed, side))
        if found == 4:
            break
    assert found == 4
