"""mfx_db_join_completeness / mfx_db_join_spectrum on the device (csrc/mfx_join.hip: mfx_join_kernel; csrc/mfx_db_join.cpp: the windows' driver).
Every result is compared `==` with two references: the oracle applied to the numpy arrays (oracle.pyoracle.completeness_piece per piece,
tests/spectrum_ref.image) and the table route on a full index loaded from the same two files (Evaluator.completeness_pieces,
Index.spectrum).  readK is an integer, so the fp64 sums are exact in any order and `==` is the right comparison.

The sizes are the smallest at which the code can go wrong: sides of 0, 1 and around one block of 4096 k-mers up to three blocks and a
piece, an equal pair on every lane and tile boundary of the merged order, windows (MFX_MERGE_RANGE) of one block first k-mer each, about
a quarter block, under a block, and everything.

k = 2 (2k < 6: the piece shift is 0): mfx_db_write_flat takes such a file (checked: it writes a sorted file of 4^2 k-mers at the most)
and the join is compared with the oracles; no table is built for it here (the table route is not part of what k = 2 adds)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import spectrum_ref as sr
from tests import stream_worlds as sw
from tests.test_join_cpu import boundary_world

pytestmark = pytest.mark.gpu

TOP = 2**32 - 1
BIG = 3 * 4096 + 17
_cache = {}
PROB = ([1, 1, 2, 0, 3, 3, 5], [0.5, 1.0, 0.25, 0.0, 0.75, 1.0, 0.125])      # rows for read counts 1 .. 7, a probK of 0 among them


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _want_completeness(k, peak, prob, read, asm):
    p = po.Params(k, peak, *(prob or (None, None)))
    shift = max(2 * k - 6, 0)
    rp, ap = (read[0] >> np.uint64(shift)) & np.uint64(63), (asm[0] >> np.uint64(shift)) & np.uint64(63)
    t, u = np.zeros(64), np.zeros(64)
    for piece in range(64):
        rs, as_ = rp == piece, ap == piece
        t[piece], u[piece] = po.completeness_piece(p, read[0][rs], read[1][rs], asm[0][as_], asm[1][as_])
    return t, u


def _check(m, tmp_path, k, read, asm, peak=17.3, prob=None, copies=4, max_mult=10000, lo=0, hi=TOP, table=True, tag="x"):
    """both joins of one world against the oracles and against the table route; returns (total, undrcpy, image, stats)"""
    rp, ap = str(tmp_path / (tag + "_r.mfxk")), str(tmp_path / (tag + "_a.mfxk"))
    m.db_write_flat(rp, k, read[0], read[1])
    m.db_write_flat(ap, k, asm[0], asm[1])
    return check_paths(m, k, rp, ap, read, asm, peak, prob, copies, max_mult, lo, hi, table, tag)


def check_paths(m, k, rp, ap, read, asm, peak=17.3, prob=None, copies=4, max_mult=10000, lo=0, hi=TOP, table=True, tag="x"):
    """... of two files that exist, whoever wrote them: rp holds the arrays read, ap the arrays asm"""
    kp = m.KParams(peak, *(prob or (None, None)))
    t, u, st = m.db_join_completeness(rp, ap, kp, with_stats=True, min_count=lo, max_count=hi)
    wt, wu = _want_completeness(k, peak, prob, read, asm)
    print("completeness", tag, float(t.sum()), float(wt.sum()), float(u.sum()), float(wu.sum()), st)
    n_both = len(np.intersect1d(read[0], asm[0]))
    assert (st["n_read"], st["n_asm"], st["n_both"]) == (len(read[0]), len(asm[0]), n_both), st
    assert np.array_equal(t, wt) and np.array_equal(u, wu), (tag, np.flatnonzero(t != wt), np.flatnonzero(u != wu))
    img, n, st2 = m.db_join_spectrum(rp, ap, copies=copies, max_mult=max_mult, min_count=lo, max_count=hi, with_entries=True, with_stats=True)
    wimg = sr.image(read, asm, copies, max_mult, lo, hi)
    print("spectrum", tag, n, int(wimg.sum()), st2)
    assert np.array_equal(img, wimg), (tag, np.argwhere(img != wimg)[:8])
    assert n == int(wimg.sum()) and (st2["n_read"], st2["n_asm"], st2["n_both"], st2["windows"]) == (len(read[0]), len(asm[0]), n_both, st["windows"])
    if table:
        ix = m.Index(k, len(read[0]) + len(asm[0]) + 64)
        ix.load_db(rp, 0, lo, hi)
        ix.load_db(ap, 1)
        timg, tn = ix.spectrum(copies, max_mult, with_entries=True)
        assert np.array_equal(img, timg) and n == tn, tag
        if lo > 1 or hi < TOP:                                     # -min / -max do not apply to -completeness: the table without them
            ix.close()
            ix = m.Index(k, len(read[0]) + len(asm[0]) + 64)
            ix.load_db(rp, 0)
            ix.load_db(ap, 1)
        tt, tu = m.Evaluator(ix, kp).completeness_pieces()
        assert np.array_equal(t, tt) and np.array_equal(u, tu), tag
        ix.close()
    return t, u, img, st


def _asm_counts(n, seed):
    """assembly counts as assemblies have them: mostly 1 and 2, some above any -copies"""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 4, size=n).astype(np.uint32)
    if n:
        v[::11] = rng.integers(5, 40, size=len(v[::11])).astype(np.uint32)
        v[3::701] = np.uint32(2**22 - 1)                           # an escape on the asm side
    return v


def _canonical_pool(k, n, seed):
    """n distinct CANONICAL k-mers, ascending (the table route's spectrum refuses a database that is not canonical); odd k: no palindromes"""
    key = ("pool", k, n, seed)
    if key not in _cache:
        x = sw.random_keys(k, min(3 * n + 64, 4 ** k), seed)
        fwd, rc = x.copy(), np.zeros(len(x), dtype=np.uint64)
        for _ in range(k):
            rc = (rc << np.uint64(2)) | ((x & np.uint64(3)) ^ np.uint64(2))
            x = x >> np.uint64(2)
        canon = np.unique(np.minimum(fwd, rc))
        assert len(canon) >= n
        _cache[key] = np.sort(np.random.default_rng(seed).choice(canon, size=n, replace=False))
    return _cache[key]


def _pair(k, relation, nr, na, seed=0):
    """(read, asm) of the sizes asked for, the relations of tests/test_gpu_merge.py::_world: disjoint (one pool dealt out: the ranges overlap),
    identical, interleaved (about half shared), asm_in_read / read_in_asm, read_below / asm_below (all of one side under all of the other)"""
    rng = np.random.default_rng(100 * k + seed)
    if relation in ("read_below", "asm_below"):
        keys = _canonical_pool(k, nr + na, 31 + seed)
        rk, ak = (keys[:nr], keys[nr:]) if relation == "read_below" else (keys[na:], keys[:na])
    elif relation == "disjoint":
        pool = _canonical_pool(k, nr + na, 32 + seed)
        perm = rng.permutation(nr + na)
        rk, ak = np.sort(pool[perm[:nr]]), np.sort(pool[perm[nr:]])
    elif relation == "identical":
        rk = ak = _canonical_pool(k, nr, 33 + seed)
    elif relation == "interleaved":
        pool = _canonical_pool(k, 2 * max(nr, na), 34 + seed)
        rk, ak = np.sort(rng.choice(pool, size=nr, replace=False)), np.sort(rng.choice(pool, size=na, replace=False))
    else:
        big = _canonical_pool(k, max(nr, na), 35 + seed)
        small = np.sort(rng.choice(big, size=min(nr, na), replace=False))
        rk, ak = (big, small) if relation == "asm_in_read" else (small, big)
    assert (len(rk), len(ak)) == (nr, na)
    return (rk, sw.mixed_counts(len(rk), 5 + seed)), (ak, _asm_counts(len(ak), 6 + seed))


SHAPES = [
    (21, "disjoint", 0, 0), (13, "disjoint", 0, 4097), (31, "disjoint", 4095, 0), (21, "identical", 1, 1), (13, "disjoint", 1, 1),
    (31, "interleaved", 4096, 4097), (21, "asm_in_read", BIG, 4095), (13, "read_in_asm", 4095, BIG), (31, "identical", 4097, 4097),
    (21, "read_below", 4096, 4096), (13, "asm_below", 4097, 4095), (31, "interleaved", BIG, BIG), (21, "disjoint", BIG, 4096), (21, "interleaved", 1, BIG),
]


@pytest.mark.parametrize("k,relation,nr,na", SHAPES, ids=["k%d-%s-%d_%d" % s for s in SHAPES])
def test_sizes_and_relations(tmp_path, monkeypatch, k, relation, nr, na):
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    read, asm = _pair(k, relation, nr, na)
    _, _, _, st = _check(m, tmp_path, k, read, asm)
    assert st["windows"] == (1 if len(read[0]) + len(asm[0]) else 0)


@pytest.mark.parametrize("which", ["lane", "tile"])
def test_ownership_on_every_boundary(tmp_path, monkeypatch, which):
    """an equal pair on every multiple of the join's lane grain (and so of its tile) in merged order -- the constants from the library --, the
    boundary between the twins, just behind and just in front of the pair.  The piece sums weigh the read counts and every (readV, asmV) is a
    cell of the image: a pair seen twice or never changes both."""
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    per, tile = m.db_join_grain()
    grain = per if which == "lane" else tile
    for shift in (0, 1, grain - 1):
        ri, ai = boundary_world(grain, shift, 3 * tile + 5 * per + 3, seed=shift)
        pool = _canonical_pool(21, int(max(ri.max(), ai.max())) + 1, 50)        # ascending: the world's order, over every piece of k = 21
        rk, ak = pool[ri.astype(np.int64)], pool[ai.astype(np.int64)]
        read = (rk, (1 + np.arange(len(rk)) % 900).astype(np.uint32))
        asm = (ak, (1 + np.arange(len(ak)) % 5).astype(np.uint32))
        _check(m, tmp_path, 21, read, asm, peak=1.0, copies=6, max_mult=1000, tag="%s%d" % (which, shift), table=(shift == 0))


def _window_world(k, name):
    if name == "boundary":                                         # tests/test_gpu_merge.py::_boundary_world's situation: the asm database holds the read
        rk = _canonical_pool(k, 2 * 4096 + 10, 21)                 # database's second block's first k-mer -- a window boundary at MFX_MERGE_RANGE=1 --
        ak = np.setdiff1d(_canonical_pool(k, 5000, 23), rk)        # in the middle of one of its blocks
        ak = np.union1d(ak, rk[[4096, 4097, 100]])
        at = int(np.searchsorted(ak, rk[4096]))
        assert ak[at] == rk[4096] and at % 4096 not in (0, 4095)
        return (rk, sw.mixed_counts(len(rk), 1)), (ak, _asm_counts(len(ak), 2))
    return _pair(k, "interleaved", BIG, 2 * 4096 + 10, seed=4)


@pytest.mark.parametrize("k,name", [(13, "blocks"), (21, "boundary"), (31, "blocks"), (31, "boundary")])
def test_windows(tmp_path, monkeypatch, k, name):
    """MFX_MERGE_RANGE of 1 (a window per block first k-mer), 1000 and 3000: the results of the one-window run; escapes inside and outside a window"""
    m = _mfx()
    read, asm = _window_world(k, name)
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    t1, u1, img1, st1 = _check(m, tmp_path, k, read, asm, prob=PROB, tag="whole")
    assert st1["windows"] == 1
    nblocks = sum((len(x[0]) + 4095) // 4096 for x in (read, asm))
    for rng in ("1", "1000", "3000"):
        monkeypatch.setenv("MFX_MERGE_RANGE", rng)
        t, u, img, st = _check(m, tmp_path, k, read, asm, prob=PROB, tag="r" + rng, table=False)
        assert 2 <= st["windows"] <= nblocks + 1, st
        assert np.array_equal(t, t1) and np.array_equal(u, u1) and np.array_equal(img, img1), rng


def test_k2(tmp_path):
    """2k < 6: the piece is the k-mer itself"""
    m = _mfx()
    read = (np.array([0, 3, 5, 9, 15], dtype=np.uint64), np.array([20, 1, 2000, 7, 40], dtype=np.uint32))
    asm = (np.array([3, 4, 9, 14, 15], dtype=np.uint64), np.array([1, 2, 9, 1, 1], dtype=np.uint32))
    t, u, img, _ = _check(m, tmp_path, 2, read, asm, peak=10.0, copies=2, max_mult=50, table=False)
    assert t[0] == 2.0 and t[5] == 200.0 and t[15] == 4.0 and t[4] == 0.0


COUNTS = [
    # copies, max_mult, -min, -max, -prob
    (4, 10000, 0, TOP, None),                                      # columns >= lds_cols (1024) straight into the image
    (1, 4, 0, TOP, PROB),                                          # a row of five columns: nearly every count >= max_mult
    (6, 2048, 5, 40, PROB),                                        # read-only k-mers become (0, 0), shared ones (0, a)
    (2, 65536, 2, TOP, None),
]


@pytest.mark.parametrize("copies,max_mult,lo,hi,prob", COUNTS, ids=["c%d-m%d-%d_%d-%s" % (c[0], c[1], c[2], min(c[3], 99), "prob" if c[4] else "peak") for c in COUNTS])
def test_counts_and_filters(tmp_path, monkeypatch, copies, max_mult, lo, hi, prob):
    """read counts of 1024 and more (past the LDS readK table), escapes on both sides, asm counts above -copies, columns at and above max_mult"""
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    k = 21
    (rk, rv), (ak, av) = _pair(k, "interleaved", BIG, 4097, seed=8)
    rv = rv.copy()
    rv[1::9] = (1000 + np.arange(len(rv[1::9])) * 7).astype(np.uint32)          # 1000 .. : both sides of 1024, of 2048 and of 10000
    rv[2::9] = 3
    assert (rv >= 1024).sum() > 100 and (rv >= 2**22 - 1).sum() > 3 and (av > 6).sum() > 100 and (av >= 2**22 - 1).sum() > 0
    if lo > 1:
        shared = np.isin(rk, ak)
        out = (rv < lo) | (rv > hi)
        assert (out & shared).sum() > 10 and (out & ~shared).sum() > 10
        if prob:                                                   # the filter, wrongly applied to -completeness, would change it
            keep = ~out
            assert not np.array_equal(_want_completeness(k, 17.3, prob, (rk[keep], rv[keep]), (ak, av))[0], _want_completeness(k, 17.3, prob, (rk, rv), (ak, av))[0])
    _check(m, tmp_path, k, (rk, rv), (ak, av), prob=prob, copies=copies, max_mult=max_mult, lo=lo, hi=hi)


def test_spectrum_aggregated_form(tmp_path, monkeypatch):
    """MFX_SPECTRUM_AGG=1: the wave-aggregated bins (mfx_spec_count<true>) give the same image"""
    m = _mfx()
    monkeypatch.setenv("MFX_SPECTRUM_AGG", "1")
    read, asm = _pair(21, "interleaved", BIG, 4097, seed=8)
    _check(m, tmp_path, 21, read, asm, table=False)


def test_damaged_block_hands_out_nothing(tmp_path, monkeypatch):
    """a count field of a block zeroed, as tests/test_gpu_merge.py::test_failure_leaves_nothing makes it: MFX_E_FORMAT naming the file, the
    outputs as they were -- in the first window and in a later one"""
    import ctypes as C
    from merfin_amd.binding import DbJoinOpts
    m = _mfx()
    L = m.load_library()
    k = 15
    (rk, rv), (ak, av) = _pair(k, "interleaved", BIG, 4096, seed=5)
    good, other = str(tmp_path / "good.mfxk"), str(tmp_path / "other.mfxk")
    m.db_write_flat(good, k, rk, rv)
    m.db_write_flat(other, k, ak, av)
    with open(good, "rb") as f:
        data = bytearray(f.read())
    n, nesc, nblocks, d = sw.directory(bytes(data))
    for block in (0, 2):
        bad = bytearray(data)
        first, off, kb, vb = d[block]
        vw = off + ((4096 - 1) * kb + 63) // 64 * 8
        word = int.from_bytes(bad[vw:vw + 8], "little") & ~((1 << vb) - 1)      # the block's first record's count field
        bad[vw:vw + 8] = word.to_bytes(8, "little")
        path = str(tmp_path / ("damaged%d.mfxk" % block))
        with open(path, "wb") as f:
            f.write(bytes(bad))
        for rng in (None, "1"):
            if rng is None:
                monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
            else:
                monkeypatch.setenv("MFX_MERGE_RANGE", rng)
            for r, a in ((path, other), (other, path)):
                o = DbJoinOpts(0, 0, TOP, 17.3, 0, None, None, 4, 100)
                t, u = np.full(64, -1.0), np.full(64, -2.0)
                img, cnt = np.full(6 * 101, 77, dtype=np.uint64), C.c_uint64(77)
                f64p, u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
                rc = L.mfx_db_join_completeness(r.encode(), a.encode(), C.byref(o), t.ctypes.data_as(f64p), u.ctypes.data_as(f64p), None)
                msg = L.mfx_last_error().decode()
                assert rc == -7 and "damaged%d.mfxk" % block in msg and "a count of zero" in msg, (rc, msg)
                assert (t == -1.0).all() and (u == -2.0).all()
                rc = L.mfx_db_join_spectrum(r.encode(), a.encode(), C.byref(o), img.ctypes.data_as(u64p), C.byref(cnt), None)
                assert rc == -7 and "damaged%d.mfxk" % block in L.mfx_last_error().decode()
                assert (img == 77).all() and cnt.value == 77
