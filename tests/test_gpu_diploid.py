"""mfx_db_diploid on the device (csrc/mfx_diploid.hip: the pair-run kernel and mfx_join_kernel with the two-assembly consumer; csrc/mfx_db_join.cpp:
the windows' driver).  Every result is compared `==` with three references: the numpy reference of tests/diploid_ref.py, the host walk
(mfx_db_diploid_host: the text the kernels run) and the chain of existing calls the pass replaces -- db_merge([hap1, hap2]) -> M, then
db_join_spectrum(reads, M) for the cn image and its entry count, and db_join_completeness on hap1, hap2 and M for the piece sums.  readK is
an integer, so the fp64 sums are exact in any order and `==` is the right comparison.

The sizes are the smallest at which the code can go wrong: roles of 0, 1 and around one block of 4096 k-mers up to three blocks and a piece,
a k-mer of all three inputs on every lane and tile boundary of both merged orders, windows (MFX_MERGE_RANGE) of under a block and everything."""
import shutil

import numpy as np
import pytest

from tests import diploid_ref as dr
from tests import stream_worlds as sw
from tests.test_diploid_cpu import BIG, EMPTY, PROB, TOP, asm_counts, assert_boundaries_hit, boundary_cases, diploid_boundary_world, read_counts

pytestmark = pytest.mark.gpu


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _write(m, tmp_path, k, world, tag):
    paths = [str(tmp_path / ("%s_%s.mfxk" % (tag, name))) for name in ("r", "h1", "h2")]
    for p, (keys, vals) in zip(paths, world):
        m.db_write_flat(p, k, keys, vals)
    return paths


def _check(m, tmp_path, k, world, peak=17.3, prob=None, copies=4, max_mult=10000, lo=0, hi=TOP, chain=True, host=True, tag="x", paths=None):
    """one call against the numpy reference, the host walk and the chain; returns the call's result"""
    rp, p1, p2 = paths or _write(m, tmp_path, k, world, tag)
    kp = m.KParams(peak, *(prob or (None, None)))
    kw = dict(copies=copies, max_mult=max_mult, min_count=lo, max_count=hi)
    got = m.db_diploid(rp, p1, p2, kparams=kp, **kw)
    st = got["stats"]
    print("diploid", tag, got["n_entries"], {x: st[x] for x in ("solid", "n_read", "n_hap1", "n_hap2", "n_shared", "windows")}, st["both"])
    want = dr.diploid(*world, k, copies=copies, max_mult=max_mult, lo=lo, hi=hi, peak=peak, prob=prob)
    assert dr.same(got, want) is None, (tag, dr.same(got, want))
    assert np.array_equal(got["asm_img"].sum(axis=0), got["cn_img"].sum(axis=0)) and st["hap1"]["distinct"] == st["n_hap1"] and st["hap2"]["distinct"] == st["n_hap2"]
    if host:
        walk = m.db_diploid_host(*world, k, kparams=kp, **kw)
        assert dr.same(got, walk) is None, (tag, dr.same(got, walk))
    if chain:
        mp = str(tmp_path / (tag + "_M.mfxk"))
        if p2 == p1:                                               # (the chain's merge is given a second name for the same bytes)
            p2 = str(tmp_path / (tag + "_h1_again.mfxk"))
            shutil.copyfile(p1, p2)
        m.db_merge([p1, p2], mp)
        img, n = m.db_join_spectrum(rp, mp, with_entries=True, **kw)
        assert np.array_equal(got["cn_img"], img) and got["n_entries"] == n, (tag, np.argwhere(got["cn_img"] != img)[:8])
        for i, ap in enumerate((p1, p2, mp)):
            t, u = m.db_join_completeness(rp, ap, kp)
            assert np.array_equal(got["total"], t) and np.array_equal(got["undrcpy"][i], u), (tag, i)
    return got


def _related(pool, relation, base, n, rng):
    """n k-mers of the ascending pool in `relation` to the ascending k-mers `base` (the relations of tests/test_gpu_join.py::_pair)"""
    third = len(pool) // 3
    if relation == "identical":
        assert n == len(base)
        return base
    if relation == "below":                                        # all of them under all of base (base comes from the middle third)
        return np.sort(rng.choice(pool[:third], size=n, replace=False))
    if relation == "above":
        return np.sort(rng.choice(pool[2 * third:], size=n, replace=False))
    outside = np.setdiff1d(pool, base)
    if relation == "disjoint":                                     # the ranges overlap
        return np.sort(rng.choice(outside, size=n, replace=False))
    if relation == "inside":
        return np.sort(rng.choice(base, size=n, replace=False))
    if relation == "around":
        return np.union1d(base, rng.choice(outside, size=n - len(base), replace=False))
    shared = min(n // 2, len(base))                                # interleaved: about half shared
    return np.union1d(rng.choice(base, size=shared, replace=False), rng.choice(outside, size=n - shared, replace=False))


_pools = {}


def world3(k, rel2, relr, anchor, nr, n1, n2, seed=0):
    """hap1 from the middle of a pool, hap2 in relation rel2 to hap1, the reads in relation relr to hap1 (anchor 1) or hap2 (anchor 2)"""
    if k not in _pools:
        _pools[k] = sw.random_keys(k, 9 * BIG, 900 + k)
    pool = _pools[k]
    rng = np.random.default_rng(100 * k + seed)
    third = len(pool) // 3
    k1 = np.sort(rng.choice(pool[third:2 * third], size=n1, replace=False))
    k2 = _related(pool, rel2, k1, n2, rng)
    rk = _related(pool, relr, k1 if anchor == 1 else k2, nr, rng)
    assert (len(rk), len(k1), len(k2)) == (nr, n1, n2)
    return (rk, read_counts(nr, 5 + seed)), (k1, asm_counts(n1, 6 + seed)), (k2, asm_counts(n2, 7 + seed))


SHAPES = [
    # k, hap2 to hap1, reads to their anchor, anchor, reads, hap1, hap2
    (21, "disjoint", "disjoint", 1, 0, 0, 0), (13, "disjoint", "disjoint", 1, 0, 4097, 1), (31, "disjoint", "disjoint", 2, 4095, 0, 4096), (21, "identical", "identical", 1, 1, 1, 1),
    (13, "disjoint", "disjoint", 1, 1, 1, 1), (31, "interleaved", "interleaved", 1, 4096, 4097, 4095), (21, "inside", "around", 1, BIG, 4096, 4095),
    (13, "around", "inside", 2, 4095, 4097, BIG), (31, "identical", "identical", 2, 4097, 4097, 4097), (21, "below", "above", 1, 4096, 4096, 4096),
    (13, "above", "below", 1, 4097, 4095, 1), (31, "interleaved", "interleaved", 2, BIG, BIG, BIG), (21, "disjoint", "interleaved", 2, BIG, 0, 4096),
    (21, "interleaved", "inside", 2, 1, 4097, BIG), (31, "below", "interleaved", 1, 4097, BIG, 0),
]


@pytest.mark.parametrize("k,rel2,relr,anchor,nr,n1,n2", SHAPES, ids=["k%d-%s-%s%d-%d_%d_%d" % s for s in SHAPES])
def test_sizes_and_relations(tmp_path, monkeypatch, k, rel2, relr, anchor, nr, n1, n2):
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    got = _check(m, tmp_path, k, world3(k, rel2, relr, anchor, nr, n1, n2))
    assert got["stats"]["windows"] == (1 if nr + n1 + n2 else 0)


@pytest.mark.parametrize("case", range(12))
def test_ownership_on_every_boundary(tmp_path, monkeypatch, case):
    """a k-mer of all three inputs on every multiple of the lane grain and of the tile of the join's merged order and of the pair step's, the
    boundary between the twins, just behind and just in front of them: a k-mer seen twice or never changes the images, the counters and the sums"""
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    order, grain, shift = boundary_cases()[case]
    per, tile = m.db_join_grain()
    world = diploid_boundary_world(grain, shift, 3 * tile + 5 * per + 3, order, seed=shift)
    assert_boundaries_hit(world, grain, shift, order)
    _check(m, tmp_path, 21, world, peak=1.0, copies=6, max_mult=1000, chain=(shift == 0), tag="%s%d_%d" % (order, grain, shift))


def _window_world(k):
    """the reads' second block's first k-mer -- a window boundary at MFX_MERGE_RANGE=3000 -- held by both assemblies in the middle of a block
    of theirs; hap2 ends under the reads' third block, so the last windows hold no record of it"""
    pool = sw.random_keys(k, 6 * BIG, 300 + k)
    rng = np.random.default_rng(k)
    rk = np.sort(rng.choice(pool, size=2 * 4096 + 10, replace=False))
    k1 = np.union1d(rng.choice(pool, size=5000, replace=False), rk[[4096, 4097, 100]])
    low = pool[pool < rk[2 * 4096]]
    k2 = np.union1d(rng.choice(low, size=3000, replace=False), rk[[4096, 50]])
    for keys in (k1, k2):
        at = int(np.searchsorted(keys, rk[4096]))
        assert keys[at] == rk[4096] and at % 4096 not in (0, 4095)
    return (rk, read_counts(len(rk), 1)), (k1, asm_counts(len(k1), 2)), (k2, asm_counts(len(k2), 3))


@pytest.mark.parametrize("k", [13, 21, 31])
def test_windows(tmp_path, monkeypatch, k):
    """MFX_MERGE_RANGE=3000: several windows, a k-mer of all three inputs at a window's lo, a window without a record of hap2; the results of the
    one-window run"""
    m = _mfx()
    world = _window_world(k)
    plan = m.db_merge_plan([x[0][::4096] for x in world], [len(x[0]) for x in world], k, 3000)
    los = [w[0] for w in plan]
    triple = np.intersect1d(np.intersect1d(world[0][0], world[1][0]), world[2][0])
    assert len(plan) >= 3 and set(triple.tolist()) & set(los)
    assert any(((world[0][0] >= lo) & (world[0][0] < hi)).any() and not ((world[2][0] >= lo) & (world[2][0] < hi)).any() for lo, hi, _, _ in plan)
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    paths = _write(m, tmp_path, k, world, "w")
    one = _check(m, tmp_path, k, world, prob=PROB, tag="whole", paths=paths)
    assert one["stats"]["windows"] == 1
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    many = _check(m, tmp_path, k, world, prob=PROB, tag="r3000", paths=paths, host=False)
    assert many["stats"]["windows"] == len([w for w in plan if w[2]]) >= 3
    assert dr.same(many, one) is None


COUNTS = [
    # copies, max_mult, -min, -max, -prob
    (4, 10000, 0, TOP, None),                                      # 10 rows: lds_cols 512, the columns from there on straight into the image
    (1, 4, 0, TOP, PROB),                                          # rows of five columns: nearly every count >= max_mult
    (6, 2048, 2, 50, PROB),                                        # 12 rows; read-only k-mers become no entry, assembly k-mers column 0
    (1, 65536, 2, TOP, None),                                      # 7 rows: lds_cols 1024
]


@pytest.mark.parametrize("copies,max_mult,lo,hi,prob", COUNTS, ids=["c%d-m%d-%d_%d-%s" % (c[0], c[1], c[2], min(c[3], 99), "prob" if c[4] else "peak") for c in COUNTS])
def test_counts_and_filters(tmp_path, monkeypatch, copies, max_mult, lo, hi, prob):
    """read counts on both sides of lds_cols (512 and 1024), of the readK table (1024) and of max_mult, escapes (2^22 - 1 and 2^32 - 1) in every
    role, assembly counts above -copies"""
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    (rk, rv), h1, h2 = world3(21, "interleaved", "interleaved", 1, BIG, 4097, 4096, seed=8)
    rv = rv.copy()
    rv[3::9] = (508 + np.arange(len(rv[3::9])) % 8).astype(np.uint32)           # 508 .. 515
    rv[5::9] = (1020 + np.arange(len(rv[5::9])) % 8).astype(np.uint32)          # 1020 .. 1027
    for v in (rv, h1[1], h2[1]):
        assert (v == 2**22 - 1).sum() > 0 and (v == TOP).sum() > 0
    assert (rv >= 1024).sum() > 100 and (h1[1] > 6).sum() > 100
    _check(m, tmp_path, 21, ((rk, rv), h1, h2), prob=prob, copies=copies, max_mult=max_mult, lo=lo, hi=hi)


def test_aggregated_form(tmp_path, monkeypatch):
    """MFX_SPECTRUM_AGG=1: the wave-aggregated bins (mfx_spec_count<true>) give the same images"""
    m = _mfx()
    world = world3(21, "interleaved", "interleaved", 2, BIG, 4097, 4097, seed=9)
    paths = _write(m, tmp_path, 21, world, "agg")
    monkeypatch.delenv("MFX_SPECTRUM_AGG", raising=False)
    plain = _check(m, tmp_path, 21, world, tag="plain", paths=paths, chain=False)
    monkeypatch.setenv("MFX_SPECTRUM_AGG", "1")
    agg = _check(m, tmp_path, 21, world, tag="agg", paths=paths)
    assert dr.same(agg, plain) is None


def test_min_max_move_the_images_not_the_qv(tmp_path, monkeypatch):
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    world = world3(21, "interleaved", "interleaved", 1, BIG, 4097, 4095, seed=10)
    paths = _write(m, tmp_path, 21, world, "mm")
    raw = _check(m, tmp_path, 21, world, tag="raw", paths=paths, chain=False)
    cut = _check(m, tmp_path, 21, world, lo=2, hi=50, tag="cut", paths=paths)
    for x in dr.NAMES:
        assert all(cut["stats"][x][f] == raw["stats"][x][f] for f in ("distinct", "total", "only_distinct", "only_total")), x
        assert cut["stats"][x]["found"] < raw["stats"][x]["found"], x
    assert cut["stats"]["solid"] < raw["stats"]["solid"]
    assert not np.array_equal(cut["asm_img"], raw["asm_img"]) and not np.array_equal(cut["cn_img"], raw["cn_img"])
    assert np.array_equal(cut["total"], raw["total"]) and np.array_equal(cut["undrcpy"], raw["undrcpy"])      # (-min / -max do not apply to -completeness)


def test_same_file_twice_and_nothing(tmp_path, monkeypatch):
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    reads, h1, _ = world3(21, "identical", "interleaved", 1, 4097, BIG, BIG, seed=11)
    rp, p1, _ = _write(m, tmp_path, 21, (reads, h1, EMPTY), "same")
    got = _check(m, tmp_path, 21, (reads, h1, h1), tag="same", paths=(rp, p1, p1))
    assert got["asm_img"][1].sum() == 0 and got["asm_img"][2].sum() == 0 and got["stats"]["n_shared"] == BIG
    none = _check(m, tmp_path, 21, (EMPTY, EMPTY, EMPTY), tag="none")
    assert none["n_entries"] == 0 and none["stats"]["windows"] == 0 and not none["asm_img"].any() and not none["total"].any()
    _check(m, tmp_path, 21, (reads, EMPTY, EMPTY), tag="reads_only")
    _check(m, tmp_path, 21, (EMPTY, h1, EMPTY), tag="hap1_only")


def test_second_run_gives_equal_bytes(tmp_path, monkeypatch):
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    world = world3(31, "interleaved", "interleaved", 2, BIG, 4097, BIG, seed=12)
    paths = _write(m, tmp_path, 31, world, "twice")
    kw = dict(kparams=m.KParams(17.3, *PROB), copies=6, max_mult=100)
    a, b = m.db_diploid(*paths, **kw), m.db_diploid(*paths, **kw)
    for key in ("asm_img", "cn_img", "total", "undrcpy"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["n_entries"] == b["n_entries"] and {x: a["stats"][x] for x in a["stats"] if not x.startswith("t_")} == {x: b["stats"][x] for x in b["stats"] if not x.startswith("t_")}
