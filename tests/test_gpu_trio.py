"""mfx_db_trio, mfx_db_trio_hist and mfx_db_histogram on the device (csrc/mfx_trio.hip: the role tag, the histogram pass, the classify pass
with its two compactions; csrc/mfx_db_trio.cpp: the windows' driver and the two streamed writers).  Every output file is compared byte for byte
with mfx_db_write_flat of the numpy reference (tests/trio_ref.py) and with the chain of existing calls (db_merge_except, db_merge,
db_merge intersect), the image and the statistics with ==; the inputs are unchanged afterwards and a second run gives the same bytes.
The sizes are the smallest at which the code can go wrong: databases of 0, 1 and around one block of 4096 k-mers up to five blocks, merged
positions around a round (256) and a tile (2048) of the classify kernel, 4096 and 4097 survivors, counts around the LDS column bound."""
import os

import numpy as np
import pytest

from tests import stream_worlds as sw
from tests import trio_ref as tr
from tests.test_gpu_merge import _bytes, _write

pytestmark = pytest.mark.gpu

KS = (15, 21, 31)
CUTS = ((1, 1, 1), (2, 3, 2), (2**32 - 1, 2**32 - 1, 2**32 - 1))      # the last one: above every count of sets() -- both outputs empty
NO_CHILD_PAT = (4097, 20000, 4096, 4095, 0, 1)              # pat's size beside mat's tr.SIZES[case] where there is no child
VALLEYS = (9, 6, 9)                                           # of the three rows of tr.auto_world(), max_mult 100 (asserted on the CPU below)


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _files(m, tmp_path, k, mat, pat, child, tag):
    return [None if d is None else _write(m, tmp_path / ("%s_%s.mfxk" % (tag, r)), k, d[0], d[1]) for r, d in (("mat", mat), ("pat", pat), ("child", child))]


def check(m, tmp_path, k, mat, pat, child, cuts, tag="x", max_mult=10000, chain=True):
    """one db_trio with explicit cutoffs against the reference and the chain; returns the stats"""
    tm, tp, tc = cuts
    pm, pp, pc = _files(m, tmp_path, k, mat, pat, child, tag)
    before = [_bytes(p) for p in (pm, pp, pc) if p]
    (ak, av), (bk, bv), _, want = tr.reference(mat, pat, child, tm, tp, tc, max_mult)
    want_a = _bytes(_write(m, tmp_path / (tag + "_wantA.mfxk"), k, ak, av))
    want_b = _bytes(_write(m, tmp_path / (tag + "_wantB.mfxk"), k, bk, bv))
    oa, ob = str(tmp_path / (tag + "_A.mfxk")), str(tmp_path / (tag + "_B.mfxk"))
    st = m.db_trio(pm, pp, pc, oa, ob, cut_mat=tm, cut_pat=tp, cut_child=tc if pc else 0, max_mult=max_mult)
    what = (k, cuts, len(mat[0]), len(pat[0]), None if child is None else len(child[0]), st)
    assert not os.path.exists(oa + ".blocks") and not os.path.exists(ob + ".blocks")
    assert _bytes(oa) == want_a, what
    assert _bytes(ob) == want_b, what
    assert {n: st[n] for n in tr.COUNTERS} == want, what
    assert (st["cut_mat"], st["cut_pat"], st["cut_child"]) == (tm, tp, tc if pc else 0) and (st["auto_mat"], st["auto_pat"], st["auto_child"], st["hist_pass"]) == (0, 0, 0, 0)
    assert [_bytes(p) for p in (pm, pp, pc) if p] == before
    if chain:
        assert _bytes(tr.chain(m, tmp_path, pm, pp, pc, str(tmp_path / "chainA.mfxk"), tm, tc)) == want_a, what
        assert _bytes(tr.chain(m, tmp_path, pp, pm, pc, str(tmp_path / "chainB.mfxk"), tp, tc)) == want_b, what
    os.remove(oa); os.remove(ob)
    m.db_trio(pm, pp, pc, oa, ob, cut_mat=tm, cut_pat=tp, cut_child=tc if pc else 0, max_mult=max_mult)      # a second run: the same bytes
    assert _bytes(oa) == want_a and _bytes(ob) == want_b
    return st


@pytest.mark.parametrize("with_child", [True, False])
@pytest.mark.parametrize("case", range(6))
def test_explicit_cutoffs_sizes_roles_and_k(tmp_path, monkeypatch, case, with_child):
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")             # several windows
    k = KS[case % 3]
    # (every size takes every role once, with and without a child; no pair of sizes here fits one window)
    mat, pat, child = tr.sets(k, tr.roles(case) if with_child else (tr.SIZES[case], NO_CHILD_PAT[case], 0), 300 + case)
    for c, cuts in enumerate(CUTS):
        st = check(m, tmp_path, k, mat, pat, child if with_child else None, cuts, tag="c%d" % c)
        assert st["windows"] > 1
        if c == 2:
            assert st["n_a"] == 0 and st["n_b"] == 0


def test_knob_unset_one_window(tmp_path, monkeypatch):
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    mat, pat, child = tr.sets(31, (20000, 4097, 4095), 41)
    assert check(m, tmp_path, 31, mat, pat, child, (2, 3, 2))["windows"] == 1
    assert check(m, tmp_path, 31, mat, pat, None, (1, 1, 1), tag="y")["windows"] == 1
    # the largest 31-mers: the tagged key uses all 64 bits
    top = np.array([2**62 - 3, 2**62 - 2, 2**62 - 1], dtype=np.uint64)
    three = np.array([3, 3, 3], dtype=np.uint32)
    st = check(m, tmp_path, 31, (top, three), (top[1:2], three[:1]), (top, three + 1), (1, 1, 1), tag="top")
    assert (st["n_a"], st["n_b"], st["n_both"]) == (2, 0, 1)


def _placed(p):
    """p k-mers of mat alone, then T1 held by all three, T2 by mat and child, T3 by pat and child, T4 by pat alone, each followed by a
    filler of mat: T1's records stand at the merged positions p, p + 1, p + 2"""
    fill = (np.arange(p, dtype=np.uint64) + 1) * 16
    t = fill[-1] + 16 + np.arange(4, dtype=np.uint64) * 32
    after = t + 8
    mk = np.sort(np.concatenate([fill, t[[0, 1]], after]))
    mat = (mk, np.full(len(mk), 5, dtype=np.uint32))
    pat = (t[[0, 2, 3]], np.array([7, 2, 9], dtype=np.uint32))
    child = (t[[0, 1, 2]], np.array([4, 3, 6], dtype=np.uint32))
    return mat, pat, child


@pytest.mark.parametrize("around", [256, 2048, 4096])
def test_records_of_one_kmer_across_rounds_and_tiles(tmp_path, monkeypatch, around):
    """the three records of one k-mer, and the two of the next ones, at every offset around a round's, a tile's and two tiles' end"""
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)      # one window: the merged positions are the ones built here
    for p in range(around - 6, around + 2):
        mat, pat, child = _placed(p)
        st = check(m, tmp_path, 21, mat, pat, child, (1, 1, 1), tag="p", chain=p == around - 1)
        assert (st["n_both"], st["n_a"], st["n_b"], st["windows"]) == (1, 1, 1, 1)      # T1; A = {T2}; B = {T3}: the child lacks T4 and the fillers
        st = check(m, tmp_path, 21, mat, pat, None, (1, 1, 1), tag="q", chain=False)
        assert (st["n_both"], st["n_a"], st["n_b"]) == (1, p + 5, 2)


def test_a_kmer_at_a_windows_lo(tmp_path, monkeypatch):
    """the first k-mer of mat's second block is a window's lo; pat and child hold it in the middle of their only block"""
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    mk = sw.random_keys(21, 2 * 4096 + 100, 71)
    lo = mk[4096]
    plan = m.db_merge_plan([mk[::4096]], [len(mk)], 21, 3000)
    assert any(w[0] == int(lo) for w in plan)
    others = np.setdiff1d(sw.random_keys(21, 600, 72), mk)
    for held_by_pat in (True, False):
        pk = np.unique(np.concatenate([others[::2], mk[4096:4097] if held_by_pat else mk[:0]]))
        ck = np.unique(np.concatenate([others[1::2], mk[4000:4200]]))
        mat = (mk, np.full(len(mk), 4, dtype=np.uint32))
        pat = (pk, np.full(len(pk), 6, dtype=np.uint32))
        child = (ck, np.full(len(ck), 3, dtype=np.uint32))
        assert 0 < np.searchsorted(pk, lo) < len(pk) - 1 and 0 < np.searchsorted(ck, lo) < len(ck) - 1
        st = check(m, tmp_path, 21, mat, pat, child, (1, 1, 1), tag="lo%d" % held_by_pat)
        assert st["windows"] > 1 and st["n_both"] == int(held_by_pat)


def test_carries_cross_windows_without_survivors(tmp_path, monkeypatch):
    """windows that feed A only, then B only, then A again: each writer's carry waits through windows that add nothing to it"""
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    low = sw.random_keys(10, 5000, 81)                         # below 4^10
    mid = sw.random_keys(10, 5000, 82) + np.uint64(1 << 24)
    high = sw.random_keys(10, 5000, 83) + np.uint64(1 << 28)
    mat = (np.concatenate([low, high]), np.full(10000, 2, dtype=np.uint32))
    pat = (mid, np.full(5000, 3, dtype=np.uint32))
    st = check(m, tmp_path, 21, mat, pat, None, (1, 1, 1))
    assert st["windows"] >= 3 and (st["n_a"], st["n_b"]) == (10000, 5000)


@pytest.mark.parametrize("n", [4096, 4097])
def test_a_block_and_one_more_survivor(tmp_path, monkeypatch, n):
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    keys = sw.random_keys(21, n + 1, 90 + n)
    mat = (keys[:n], np.full(n, 2, dtype=np.uint32))
    pat = (keys[n:], np.full(1, 2, dtype=np.uint32))
    st = check(m, tmp_path, 21, mat, pat, None, (1, 1, 1), tag="a")
    assert (st["n_a"], st["n_b"]) == (n, 1)
    st = check(m, tmp_path, 21, pat, mat, None, (1, 1, 1), tag="b")
    assert (st["n_a"], st["n_b"]) == (1, n)


def test_escaped_counts(tmp_path, monkeypatch):
    """counts that take the escape list in every input; the count written is the smaller of two such counts"""
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    (mk, _), (pk, _), (ck, _) = tr.sets(21, (9000, 5000, 9000), 95)
    mat, pat, child = (mk, sw.mixed_counts(len(mk), 1)), (pk, sw.mixed_counts(len(pk), 2)), (ck, sw.mixed_counts(len(ck), 3))
    for cuts in ((1, 1, 1), (2**22 - 1, 30, 2)):
        st = check(m, tmp_path, 21, mat, pat, child, cuts, tag="e%d" % cuts[1])
        assert st["n_a"] > 0 and st["n_b"] > 0
    (ak, av), _, _, _ = tr.reference(mat, pat, child, 1, 1, 1)
    assert (av >= 2**22 - 1).any()                             # an escaped count is written


def _hist_world():
    """counts on both sides of max_mult = 4 and 16, of the LDS column bound 2048, and far beyond"""
    (mk, _), (pk, _), (ck, _) = tr.sets(21, (20000, 4097, 12000), 97)
    rng = np.random.default_rng(98)
    special = np.array([1, 3, 4, 5, 15, 16, 17, 2047, 2048, 2049, 9999, 10000, 10001, 2**22, 2**32 - 1], dtype=np.uint32)
    return [(k_, np.where(rng.random(len(k_)) < 0.5, rng.integers(1, 40, size=len(k_)), rng.choice(special, size=len(k_))).astype(np.uint32)) for k_ in (mk, pk, ck)]


@pytest.mark.parametrize("max_mult", [4, 16, 10000])
def test_images_and_histogram(tmp_path, monkeypatch, max_mult):
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    mat, pat, child = _hist_world()
    pm, pp, pc = _files(m, tmp_path, 21, mat, pat, child, "h")
    _, _, want, wst = tr.reference(mat, pat, child, 1, 1, 1, max_mult)
    if max_mult == 10000:
        assert want[:, 2047].all() and want[:, 2048].all() and want[:, 10000].all()      # both sides of the LDS bound, and the overflow column
    img, st = m.db_trio_hist(pm, pp, pc, max_mult=max_mult, with_stats=True)
    assert (img == want).all() and int(img[2].sum()) == len(child[0])
    assert {n: st[n] for n in ("n_mat", "n_pat", "n_child", "n_both", "n_mat_only", "n_pat_only")} == {n: wst[n] for n in ("n_mat", "n_pat", "n_child", "n_both", "n_mat_only", "n_pat_only")}
    assert st["windows"] > 1
    assert (m.db_trio_hist(pm, pp, pc, max_mult=max_mult) == img).all()      # a second run
    img2 = m.db_trio_hist(pm, pp, None, max_mult=max_mult)
    assert (img2[:2] == want[:2]).all() and not img2[2].any()
    for p, d in ((pm, mat), (pp, pat), (pc, child)):
        row, n = m.db_histogram(p, max_mult=max_mult, with_count=True)
        assert n == len(d[0]) and (row == np.bincount(np.minimum(d[1], max_mult).astype(np.int64), minlength=max_mult + 1).astype(np.uint64)).all()
        assert (row == m.db_trio_hist(pm, pp, p, max_mult=max_mult)[2]).all()
    monkeypatch.setenv("MFX_SPECTRUM_AGG", "1")               # the wave-aggregated LDS adds: the same image
    assert (m.db_trio_hist(pm, pp, pc, max_mult=max_mult) == want).all()
    empty = _write(m, tmp_path / "none.mfxk", 21, *tr.EMPTY)
    assert not m.db_histogram(empty, max_mult=max_mult).any()


def test_automatic_cutoffs(tmp_path, monkeypatch):
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    mat, pat, child = tr.auto_world()
    _, _, rows, _ = tr.reference(mat, pat, child, 1, 1, 1, 100)
    peaks = [m.spectrum_peak(r) for r in rows]                 # (host code that is not under test: a condition of this test)
    assert all(p is not None for p in peaks) and tuple(p["valley"] for p in peaks) == VALLEYS
    assert 18 <= peaks[0]["main_peak"] <= 22
    pm, pp, pc = _files(m, tmp_path, 21, mat, pat, child, "auto")
    oa, ob = str(tmp_path / "A.mfxk"), str(tmp_path / "B.mfxk")
    st, img = m.db_trio(pm, pp, pc, oa, ob, max_mult=100, with_image=True)
    assert (st["cut_mat"], st["cut_pat"], st["cut_child"]) == VALLEYS and (st["auto_mat"], st["auto_pat"], st["auto_child"], st["hist_pass"]) == (1, 1, 1, 1)
    assert (img == rows).all()
    want = check(m, tmp_path, 21, mat, pat, child, VALLEYS, tag="explicit", max_mult=100)
    assert _bytes(oa) == _bytes(str(tmp_path / "explicit_A.mfxk")) and _bytes(ob) == _bytes(str(tmp_path / "explicit_B.mfxk"))
    assert {n: st[n] for n in tr.COUNTERS} == {n: want[n] for n in tr.COUNTERS} and st["n_a"] > 0 and st["n_b"] > 0
    # one cutoff given, the others automatic; parents alone
    st = m.db_trio(pm, pp, pc, oa, ob, cut_pat=4, max_mult=100)
    assert (st["cut_mat"], st["cut_pat"], st["cut_child"], st["auto_mat"], st["auto_pat"], st["auto_child"]) == (VALLEYS[0], 4, VALLEYS[2], 1, 0, 1)
    st = m.db_trio(pm, pp, None, oa, ob, max_mult=100)
    assert (st["cut_mat"], st["cut_pat"], st["cut_child"], st["auto_child"]) == (VALLEYS[0], VALLEYS[1], 0, 0)
    (ak, av), (bk, bv), _, _ = tr.reference(mat, pat, None, VALLEYS[0], VALLEYS[1])
    assert _bytes(oa) == _bytes(_write(m, tmp_path / "w.mfxk", 21, ak, av)) and _bytes(ob) == _bytes(_write(m, tmp_path / "w.mfxk", 21, bk, bv))


def test_a_row_without_a_valley_writes_nothing(tmp_path):
    m = _mfx()
    mat, pat, child = tr.sets(21, (20000, 4097, 9000), 99, lo=1, hi=2)      # every count is 1
    pm, pp, pc = _files(m, tmp_path, 21, mat, pat, child, "flat")
    oa, ob = str(tmp_path / "A.mfxk"), str(tmp_path / "B.mfxk")
    for kw, named in (({}, pm), ({"cut_mat": 1}, pp), ({"cut_mat": 1, "cut_pat": 1}, pc)):
        with pytest.raises(m.MfxError) as e:
            m.db_trio(pm, pp, pc, oa, ob, **kw)
        assert e.value.code == m.E_NODATA and named in str(e.value) and "cut" in str(e.value)
        assert not os.path.exists(oa) and not os.path.exists(ob) and not os.path.exists(oa + ".blocks") and not os.path.exists(ob + ".blocks")
    assert m.db_trio(pm, pp, pc, oa, ob, cut_mat=1, cut_pat=1, cut_child=1)["n_a"] > 0


def test_the_same_file_twice_and_empty_inputs(tmp_path):
    m = _mfx()
    (a, b) = tr.sets(21, (4097, 100), 77)
    st = check(m, tmp_path, 21, a, a, None, (1, 1, 1), tag="same")      # equal parents: two databases of no k-mers
    assert (st["n_a"], st["n_b"], st["n_both"]) == (0, 0, 4097)
    pa = _write(m, tmp_path / "one.mfxk", 21, *a)
    oa, ob = str(tmp_path / "A.mfxk"), str(tmp_path / "B.mfxk")
    assert m.db_trio(pa, pa, None, oa, ob, cut_mat=1, cut_pat=1)["n_both"] == 4097 and m.db_probe(oa)["n_kmers"] == 0 and m.db_probe(ob)["n_kmers"] == 0
    check(m, tmp_path, 21, tr.EMPTY, tr.EMPTY, tr.EMPTY, (1, 1, 1), tag="none")
    check(m, tmp_path, 21, a, tr.EMPTY, b, (1, 1, 1), tag="nopat")
