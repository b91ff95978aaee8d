"""The block decoder of -merge and -join (csrc/mfx_merge.hip: mfx_delta_decode_kernel) on blocks the library's writer never makes: the
catalogue of tests/delta_blocks.py at forced and extreme widths (tests/damaged_blocks.py: valid_cases) through mfx_db_merge and the two
joins, and every damaged file of damaged_blocks.damages -- each must end in MFX_E_FORMAT naming the file and exactly the classes it shows,
with nothing written and nothing handed out.  The references are those of tests/test_gpu_merge.py (numpy, then mfx_db_write_flat: bytes)
and tests/test_gpu_join.py (the oracle per piece, tests/spectrum_ref.image: arrays); every comparison is ==."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import damaged_blocks as dm
from tests import delta_blocks as db
from tests import stream_worlds as sw
from tests import test_gpu_join as tj
from tests import test_gpu_merge as tm

pytestmark = pytest.mark.gpu

OPS = tm.OPS
TOP = 2**32 - 1
PAIRED = ("widths", "carry", "grid", "kbits2k", "len1", "len17", "len4095")
JOINED = ("widths", "carry", "grid")


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _arrays(kmers, counts):
    return np.array(kmers, dtype=np.uint64), np.array(counts, dtype=np.uint32)


def _interleaved(k, keys, seed):
    """a database for the library's writer that interleaves with keys and shares about half of them: every second one, the midpoints behind
    every fourth one where there is room, one k-mer in front and one behind"""
    mid = keys[1:-1:4] + (keys[2::4][:len(keys[1:-1:4])] - keys[1:-1:4]) // np.uint64(2)
    ends = [x for x in (int(keys[0]) - 1, int(keys[-1]) + 1) if 0 <= x < 4 ** k]
    new = np.setdiff1d(np.concatenate([mid, np.array(ends, dtype=np.uint64)]), keys)
    out = np.union1d(keys[::2], new)
    return out, sw.mixed_counts(len(out), seed)


def _range(monkeypatch, rng):
    for name, v in (("MFX_MERGE_RANGE", rng), ("MFX_DB_BOUNCE", "4096" if rng == "1000" else None)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    """the files the Python encoder writes, once per module: case(k, name) -> (path, k-mers, counts); other(k, name) -> the same of the
    library-written database that interleaves with it; damaged(k, name) -> (Damage, its path or paths); partner(k) -> (path, k-mers, counts)"""
    d = tmp_path_factory.mktemp("blocks")
    made, cats, dams = {}, {}, {}

    class Store:
        def names(self, k):
            if k not in cats:
                cats[k] = {c.name: c for c in dm.valid_cases(k)}
            return list(cats[k])

        def case(self, k, name):
            if ("case", k, name) not in made:
                self.names(k)
                c = cats[k][name]
                made[("case", k, name)] = (c.write(str(d / ("%s_k%d.mfxk" % (name, k)))),) + _arrays(c.kmers, c.counts)
            return made[("case", k, name)]

        def other(self, k, name):
            if ("other", k, name) not in made:
                keys, vals = _interleaved(k, self.case(k, name)[1], 3 * k)
                path = str(d / ("%s_k%d_other.mfxk" % (name, k)))
                _mfx().db_write_flat(path, k, keys, vals)
                made[("other", k, name)] = (path, keys, vals)
            return made[("other", k, name)]

        def damaged(self, k, name):
            if k not in dams:
                dams[k] = {x.name: x for x in dm.damages(k)}
            if ("damaged", k, name) not in made:
                made[("damaged", k, name)] = (dams[k][name], dams[k][name].write(d))
            return made[("damaged", k, name)]

        def partner(self, k):
            if ("partner", k) not in made:
                keys, vals = dm.partner(k)
                path = str(d / ("partner_k%d.mfxk" % k))
                _mfx().db_write_flat(path, k, keys, vals)
                made[("partner", k)] = (path, keys, vals)
            return made[("partner", k)]
    return Store()


# ---- the valid catalogue through the merge ----
@pytest.mark.parametrize("k", [15, 21, 31])
def test_merge_of_one_catalogue_file_is_the_writers_file(k, store, tmp_path, monkeypatch):
    """db_merge([file], sum): byte for byte what mfx_db_write_flat makes of the case's arrays, whatever widths the file is written at"""
    m = _mfx()
    _range(monkeypatch, None)
    names = store.names(k)
    assert len(names) == len(db.synthetic(k)) and set(PAIRED) <= set(names)
    for name in names:
        path, keys, vals = store.case(k, name)
        st = tm.check_paths(m, tmp_path, k, [path], [(keys, vals)], "sum", tag=name, load_back=False)
        assert st["n_in"] == st["n_out"] == len(keys) and st["windows"] == 1, (name, st)


@pytest.mark.parametrize("k,name", [(k, n) for k in (15, 21, 31) for n in PAIRED], ids=lambda x: str(x))
def test_merge_of_a_catalogue_file_and_a_written_one(k, name, store, tmp_path, monkeypatch):
    m = _mfx()
    _range(monkeypatch, None)
    path, keys, vals = store.case(k, name)
    opath, okeys, ovals = store.other(k, name)
    shared = len(np.intersect1d(keys, okeys))
    assert len(keys) // 2 <= shared <= len(keys) // 2 + 1 and (name == "kbits2k" or len(okeys) > shared)
    for op in OPS:
        tm.check_paths(m, tmp_path, k, [path, opath], [(keys, vals), (okeys, ovals)], op, tag=op, load_back=False)
    tm.check_paths(m, tmp_path, k, [opath, path], [(okeys, ovals), (keys, vals)], "sum", tag="swapped", load_back=False)


@pytest.mark.parametrize("rng", ["1", "1000"])
@pytest.mark.parametrize("k,name", [(k, n) for k in (15, 21, 31) for n in ("widths", "grid")], ids=lambda x: str(x))
def test_merge_of_a_catalogue_file_by_windows(k, name, rng, store, tmp_path, monkeypatch):
    """MFX_MERGE_RANGE of 1 and of 1000: blocks of every width decoded in several windows, the output loaded back through the table"""
    m = _mfx()
    _range(monkeypatch, rng)
    path, keys, vals = store.case(k, name)
    opath, okeys, ovals = store.other(k, name)
    for op in ("sum", "intersect"):
        st = tm.check_paths(m, tmp_path, k, [path, opath], [(keys, vals), (okeys, ovals)], op, tag=op, load_back=(op == "sum"))
        assert st["windows"] >= 2, st
    st = tm.check_paths(m, tmp_path, k, [path], [(keys, vals)], "sum", tag="alone", load_back=False)
    assert st["windows"] >= 2, st


def _boundary_pair(k):
    """A: one block written 3 bits wider than its narrowest, at vbits 9, whose records 1000 (L), 1999 (H - 1) and 2000 (H) hold escaped counts;
    B, for the library's writer: three blocks whose second starts at L and whose third starts at H"""
    rng = np.random.default_rng(70 + k)
    d = [int(x) for x in rng.integers(12, 20, db.BLOCK - 1)]
    d[1999] = 1
    a = db._block(50000, d)
    ac = [int(x) for x in rng.integers(1, 511, db.BLOCK)]
    for i, v in ((5, 511), (1000, 511), (1999, TOP), (2000, 70000), (3000, 1 << 22)):
        ac[i] = v
    L, H = a[1000], a[2000]
    b = [L - 8193 + 2 * i for i in range(db.BLOCK)] + [L + 2 * i for i in range(db.BLOCK)] + [H + 3 * i for i in range(100)]
    assert 0 < b[0] and b[db.BLOCK - 1] < L and b[2 * db.BLOCK - 1] < H - 1 and all(y > x for x, y in zip(b, b[1:]))
    return a, ac, np.array(b, dtype=np.uint64), (1 + np.arange(len(b)) % 7).astype(np.uint32)


@pytest.mark.parametrize("k", [21, 31])
def test_escapes_at_both_ends_of_a_window(k, tmp_path, monkeypatch):
    """escaped records of a forced-width block at exactly lo, hi - 1 and hi of a window [lo, hi) that the other input's block first k-mers
    cut: the one at lo and the one at hi - 1 are looked up in this window's slice of the escape list, the one at hi in the next window's"""
    m = _mfx()
    a, ac, bk, bv = _boundary_pair(k)
    L, H = a[1000], a[2000]
    apath, bpath = str(tmp_path / "a.mfxk"), str(tmp_path / "b.mfxk")
    written = db.encode_counts(apath, k, a, ac, lambda b, kb, vb: (kb + 3, 9))
    assert written == [(8, 9)]
    raw = db.decode_raw(apath)
    assert [raw.fields[i] for i in (1000, 1999, 2000)] == [None] * 3 and a[1999] == H - 1
    m.db_write_flat(bpath, k, bk, bv)
    plan = m.db_merge_plan([np.array(a[:1], dtype=np.uint64), bk[::db.BLOCK]], [len(a), len(bk)], k, 1)
    assert (L, H) in [(w[0], w[1]) for w in plan] and H in [w[0] for w in plan]
    ak, av = _arrays(a, ac)
    _range(monkeypatch, "1")
    for op in OPS:
        st = tm.check_paths(m, tmp_path, k, [apath, bpath], [(ak, av), (bk, bv)], op, tag=op, load_back=(op == "sum"))
        assert st["windows"] == sum(1 for w in plan if w[2]) >= 4  # (a window without a block is not counted)
    tm.check_paths(m, tmp_path, k, [bpath, apath], [(bk, bv), (ak, av)], "sum", tag="swapped", load_back=False)
    tj.check_paths(m, k, apath, bpath, (ak, av), (bk, bv), table=False, tag="read")
    tj.check_paths(m, k, bpath, apath, (bk, bv), (ak, av), table=False, tag="asm")


# ---- the valid catalogue through the join ----
@pytest.mark.parametrize("k,name", [(k, n) for k in (21, 31) for n in JOINED], ids=lambda x: str(x))
def test_join_of_a_catalogue_file_and_a_written_one(k, name, store, monkeypatch):
    """the catalogue file as the read side and as the asm side, in one window and in one per block first k-mer.  Against the oracles only: the
    catalogue's k-mers are not canonical, which the table route's spectrum refuses"""
    m = _mfx()
    path, keys, vals = store.case(k, name)
    opath, okeys, ovals = store.other(k, name)
    for rng in (None, "1"):
        _range(monkeypatch, rng)
        *_, st = tj.check_paths(m, k, path, opath, (keys, vals), (okeys, ovals), table=False, tag="read")
        assert (st["windows"] == 1) == (rng is None)
        *_, st = tj.check_paths(m, k, opath, path, (okeys, ovals), (keys, vals), prob=tj.PROB, copies=6, max_mult=2048, table=False, tag="asm")
        assert (st["windows"] == 1) == (rng is None)


# ---- damaged files ----
def _damage_names(k):
    return [d.name for d in dm.damages(k) if d.expected and d.name != "two"]


DAMAGED = [(k, n) for k in (21, 31) for n in _damage_names(k)]


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _says(msg, path, classes, silent=()):
    """the message names the file and holds the words of exactly these classes"""
    assert os.path.basename(path) in msg and not any(os.path.basename(p) in msg for p in silent), msg
    for c, text in dm.TEXT.items():
        assert (text in msg) == (c in classes), (c, msg)


def _merge_refuses(m, paths, out, bad, classes):
    before = [_bytes(p) for p in paths]
    with pytest.raises(m.MfxError) as e:
        m.db_merge(paths, out)
    assert e.value.code == -7, str(e.value)                        # MFX_E_FORMAT
    _says(str(e.value), bad, classes, [p for p in paths if p != bad])
    assert not os.path.exists(out) and not os.path.exists(out + ".blocks")
    assert [_bytes(p) for p in paths] == before


def _join_refuses(m, read, asm, bad, classes):
    """both joins through the C entry points: -7, the message, the caller's arrays as they were"""
    from merfin_amd.binding import DbJoinOpts
    lib = m.load_library()
    f64p, u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    o = DbJoinOpts(0, 0, TOP, 17.3, 0, None, None, 4, 100)
    t, u = np.full(64, -1.0), np.full(64, -2.0)
    img, cnt = np.full(6 * 101, 77, dtype=np.uint64), C.c_uint64(77)
    rc = lib.mfx_db_join_completeness(read.encode(), asm.encode(), C.byref(o), t.ctypes.data_as(f64p), u.ctypes.data_as(f64p), None)
    assert rc == -7
    _says(lib.mfx_last_error().decode(), bad, classes, [p for p in (read, asm) if p != bad])
    assert (t == -1.0).all() and (u == -2.0).all()
    rc = lib.mfx_db_join_spectrum(read.encode(), asm.encode(), C.byref(o), img.ctypes.data_as(u64p), C.byref(cnt), None)
    assert rc == -7
    _says(lib.mfx_last_error().decode(), bad, classes, [p for p in (read, asm) if p != bad])
    assert (img == 77).all() and cnt.value == 77


@pytest.mark.parametrize("k,name", DAMAGED, ids=lambda x: str(x))
def test_merge_refuses_a_damaged_file(k, name, store, tmp_path, monkeypatch):
    """as input 0 and as input 1 of two, in one window and in one per block first k-mer (where damaged_blocks.partner cuts the damaged
    file's blocks, so that a block is decoded for several windows and lost-rm-outside is found in a later window than its block's first)"""
    m = _mfx()
    d, bad = store.damaged(k, name)
    good = store.partner(k)[0]
    for rng in (None, "1"):
        _range(monkeypatch, rng)
        for i, paths in enumerate(([bad, good], [good, bad])):
            _merge_refuses(m, paths, str(tmp_path / ("out%s%d.mfxk" % (rng, i))), bad, d.expected)


@pytest.mark.parametrize("k,name", DAMAGED, ids=lambda x: str(x))
def test_join_refuses_a_damaged_file(k, name, store, monkeypatch):
    m = _mfx()
    d, bad = store.damaged(k, name)
    good = store.partner(k)[0]
    for rng in (None, "1"):
        _range(monkeypatch, rng)
        _join_refuses(m, bad, good, bad, d.expected)
        _join_refuses(m, good, bad, bad, d.expected)


@pytest.mark.parametrize("k", [21, 31])
def test_two_damaged_inputs_name_the_first(k, store, tmp_path, monkeypatch):
    """a zero count in input 0, a repeated k-mer in input 1, both in the same window: the decoder marks both inputs, the message is the
    first input's and holds that input's class alone"""
    m = _mfx()
    d, (p0, p1) = store.damaged(k, "two")
    for rng in (None, "1"):
        _range(monkeypatch, rng)
        _merge_refuses(m, [p0, p1], str(tmp_path / ("a%s.mfxk" % rng)), p0, d.expected[0])
        _merge_refuses(m, [p1, p0], str(tmp_path / ("b%s.mfxk" % rng)), p1, d.expected[1])
        _join_refuses(m, p0, p1, p0, d.expected[0])
        _join_refuses(m, p1, p0, p1, d.expected[1])


@pytest.mark.parametrize("k", [21, 31])
def test_a_stale_escape_entry_is_ignored_by_merge_and_join_and_loaded_by_the_table(k, store, tmp_path, monkeypatch):
    """one more escape-list entry that no count field refers to.  This pins PRESENT behaviour, and the consumers differ: the decoder of -merge
    and -join looks an entry up only from an escape field, so both give what the blocks' records give; the table loader inserts every
    entry of the list (load_flat_escapes), so the same file loads as its records plus the stale entry (docs/DESIGN_DETAIL.md, "Blocks
    no writer makes")."""
    m = _mfx()
    d, path = store.damaged(k, "stale")
    assert d.expected == set() and dm.classify(path) == set()
    keys, vals = _arrays(d.source.kmers, d.source.counts)
    (stale,) = set(d.escapes) - set(d.source.raw.escapes)
    assert stale[0] not in d.source.kmers
    gpath, gk, gv = store.partner(k)
    for rng in (None, "1"):
        _range(monkeypatch, rng)
        for op in OPS:
            tm.check_paths(m, tmp_path, k, [path, gpath], [(keys, vals), (gk, gv)], op, tag=op, load_back=False)
        tm.check_paths(m, tmp_path, k, [path], [(keys, vals)], "sum", tag="alone", load_back=False)
        tj.check_paths(m, k, path, gpath, (keys, vals), (gk, gv), table=False, tag="read")
        tj.check_paths(m, k, gpath, path, (gk, gv), (keys, vals), table=False, tag="asm")
    table, _ = db.expected(d.source.kmers, d.source.counts)
    table[stale[0]] = table.get(stale[0], 0) + stale[1]
    assert len(table) == len(keys) + 1
    ix = m.Index(k, len(table) + 16)
    ix.load_db(path, 0)
    ek, er, ea = ix.export()
    want = np.array(sorted(table), dtype=np.uint64)
    np.testing.assert_array_equal(ek, want)
    np.testing.assert_array_equal(er, np.array([table[x] for x in want.tolist()], dtype=np.uint32))
    assert not ea.any()
