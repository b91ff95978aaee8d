"""One window of the database calls past the first round of what loops inside it.  Production windows hold up to 2^26 merged positions;
every other test stays below about 36 000, so these paths run nowhere else:

  the offset scans   mfx_tile_scan_kernel (csrc/mfx_merge.hip) and mfx_tile_scan2_kernel (csrc/mfx_trio.hip) are one workgroup that takes
                     256 tiles a round and carries the running total to the next round in LDS (s_carry).  A tile is MFX_COMB_TILE =
                     MFX_TRIO_TILE = 2048 merged positions, so the carry is first used above 256 x 2048 = 524 288 positions and used twice
                     above 2 x 256 x 2048 = 1 048 576: the merges here have more than that (n_in), and so has the trio
  mfx_trio_hist_kernel   persistent workgroups, CUs x 4 of 256 positions, LDS bins kept from turn to turn: a workgroup takes a third turn
                     above 2 x (CUs x 4) x 256 merged positions
  mfx_join_kernel    persistent workgroups over tiles of MFX_JOIN_TILE = 2048 merged positions (db_join_grain), CUs x 4 of them for
                     -completeness and CUs x 2 for -spectrum (csrc/mfx_db_join.cpp): with CUs x 4 x 2048 + 3 x 2048 < positions < 2 x CUs x 4 x
                     2048 some workgroups of the completeness launch take a second turn and some do not, and the spectrum launch's take a
                     third
  the encoder        gets a window's survivors in one append: hundreds of blocks a launch instead of a handful

The CU count comes from the device's properties and every size condition is asserted in the test that relies on it.  MFX_MERGE_RANGE is
unset and `windows == 1` asserted throughout.  The references and the checks are those of tests/test_gpu_merge.py, tests/test_gpu_trio.py
(tests/trio_ref.py) and tests/test_gpu_join.py, unchanged; everything is compared with ==."""
import os

import numpy as np
import pytest

from tests import trio_ref as tr
from tests import test_gpu_join as tj
from tests import test_gpu_merge as tm
from tests import test_gpu_trio as tt

pytestmark = pytest.mark.gpu

SCAN_ROUND = 256                                                   # tiles a round of the one-workgroup scans
TILE = 2048                                                        # MFX_COMB_TILE, MFX_TRIO_TILE: 8 rounds of 256 positions
HIST_WG = 256                                                      # positions a turn of a workgroup of mfx_trio_hist_kernel
TOP = 2**32 - 1
_cache = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def cus():
    """the device's compute units, from torch's device properties (the import is this module's one slow step)"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _one_window(monkeypatch):
    for name in ("MFX_MERGE_RANGE", "MFX_DB_BOUNCE", "MFX_SPECTRUM_AGG"):
        monkeypatch.delenv(name, raising=False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------------------------------------------------
def _merge_world(m, k, root):
    """three databases from one pool of 1 060 000 k-mers (530 000, 530 000 and 300 000: about half of each shared with each other one),
    counts of stream_worlds.mixed_counts; their files, written once"""
    if ("merge", k) not in _cache:
        inputs = tm._world(k, "interleaved", (530000, 530000, 300000), seed=50)
        paths = [tm._write(m, os.path.join(root, "merge_k%d_%d.mfxk" % (k, i)), k, a, b) for i, (a, b) in enumerate(inputs)]
        _cache[("merge", k)] = (inputs, paths)
    return _cache[("merge", k)]


@pytest.fixture(scope="module")
def files_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("large_window"))


@pytest.mark.parametrize("k,op", [(21, "sum"), (21, "max"), (21, "min"), (21, "intersect"), (31, "sum")])
def test_merge_scan_carry_used_twice(tmp_path, monkeypatch, files_dir, k, op):
    m = _mfx()
    _one_window(monkeypatch)
    inputs, paths = _merge_world(m, k, files_dir)
    shared = len(np.intersect1d(inputs[0][0], inputs[1][0]))
    assert 0.4 * 530000 < shared < 0.6 * 530000                    # interleaved: about half shared
    st = tm.check_paths(m, tmp_path, k, paths[:2], inputs[:2], op, tag=op)
    assert st["windows"] == 1
    assert st["n_in"] > 2 * SCAN_ROUND * TILE                      # three rounds of the scan: the carry is used twice
    assert st["n_out"] > 32 * 4096                                 # and the encoder gets more than 32 blocks in one append


def _survivors_per_tile(inputs, rk):
    """of the merged run of the inputs (equal k-mers side by side): how many of the k-mers rk have their head in each tile"""
    keys = np.sort(np.concatenate([a for a, _ in inputs]))
    u, first = np.unique(keys, return_index=True)                  # the head of a k-mer: its first position in the merged run
    heads = first[np.isin(u, rk)]
    return np.bincount(heads // TILE, minlength=(len(keys) + TILE - 1) // TILE)


def test_merge_filter_leaves_tiles_of_every_fill(tmp_path, monkeypatch, files_dir):
    """a filter that drops most k-mers: the tiles' survivor numbers -- what the scan adds up -- run from none to every k-mer of a tile"""
    m = _mfx()
    _one_window(monkeypatch)
    k = 21
    inputs, _ = _merge_world(m, k, files_dir)
    (ak, av), (bk, bv) = inputs[:2]
    av, bv = av.copy(), bv.copy()
    lo_key, hi_key = ak[len(ak) // 33], ak[len(ak) // 2]           # a stretch where nothing survives, a stretch where everything does
    for keys, vals in ((ak, av), (bk, bv)):
        vals[keys < lo_key] = 1
        vals[(keys >= hi_key) & (keys < hi_key + (hi_key - lo_key) // 16)] = 2**21
    world = [(ak, av), (bk, bv)]
    cut = 100000
    rk, _, nfilt, _ = tm.reference(world, "sum", cut, TOP)
    per_tile = _survivors_per_tile(world, rk)
    assert len(per_tile) > 2 * SCAN_ROUND and per_tile.min() == 0 and per_tile.max() > TILE // 2 and nfilt > 10 * len(rk)
    assert (per_tile[:SCAN_ROUND] == 0).any() and per_tile[SCAN_ROUND:2 * SCAN_ROUND].max() > TILE // 2 and per_tile[2 * SCAN_ROUND:].sum() > 0
    st = tm._check(m, tmp_path, k, world, "sum", cut, TOP, tag="filter")
    assert st["windows"] == 1 and st["n_in"] > 2 * SCAN_ROUND * TILE and 0 < st["n_out"] < st["n_in"] // 10


def test_merge_except_a_third_file(tmp_path, monkeypatch, files_dir):
    m = _mfx()
    _one_window(monkeypatch)
    k = 21
    inputs, paths = _merge_world(m, k, files_dir)
    before = [tm._bytes(p) for p in paths]
    rk, rv, _, nsat = tm.reference(inputs[:2], "sum")
    barred = np.isin(rk, inputs[2][0])
    assert 0.1 * len(rk) < barred.sum() < 0.5 * len(rk)
    want = tm._bytes(tm._write(m, tmp_path / "want.mfxk", k, rk[~barred], rv[~barred]))
    out = str(tmp_path / "out.mfxk")
    for run in (0, 1):
        st = m.db_merge_except(paths[:2], paths[2:], out)
        assert tm._bytes(out) == want and not os.path.exists(out + ".blocks")
        assert (st["n_out"], st["n_subtracted"], st["n_filtered"], st["windows"]) == (int((~barred).sum()), int(barred.sum()), 0, 1), st
        assert st["n_saturated"] == nsat
    assert sum(len(a) for a, _ in inputs) > 2 * SCAN_ROUND * TILE  # the merged run holds the subtracted database's records too
    assert [tm._bytes(p) for p in paths] == before


# ---------------------------------------------------------------------------------------------------------------------------------------
# trio
# ---------------------------------------------------------------------------------------------------------------------------------------
TRIO_SIZES = (400000, 400000, 300000)


def _trio_world(k):
    if ("trio", k) not in _cache:
        _cache[("trio", k)] = tr.sets(k, TRIO_SIZES, 700 + k, pool=800000)
    return _cache[("trio", k)]


@pytest.mark.parametrize("cuts,with_child", [((2, 3, 2), True), ((1, 1, 1), True), ((2, 3, 2), False)], ids=["cuts232", "cuts111", "nochild"])
def test_trio_scan_carry_and_both_writers(tmp_path, monkeypatch, cuts, with_child):
    m = _mfx()
    _one_window(monkeypatch)
    k = 31
    mat, pat, child = _trio_world(k)
    positions = len(mat[0]) + len(pat[0]) + (len(child[0]) if with_child else 0)
    if with_child:
        assert positions > 2 * SCAN_ROUND * TILE                   # mfx_tile_scan2_kernel: three rounds, both carries used twice
    else:
        assert positions > SCAN_ROUND * TILE                       # (800 000 positions: two rounds)
    st = tt.check(m, tmp_path, k, mat, pat, child if with_child else None, cuts, tag="t", chain=False)
    assert st["windows"] == 1
    assert st["n_a"] > 4 * 4096 and st["n_b"] > 4 * 4096 and st["n_both"] > 4 * 4096      # several blocks an append for both writers


def test_trio_hist_workgroups_take_a_third_turn(tmp_path, monkeypatch, cus):
    """db_trio_hist and db_histogram over one window: the LDS bins of a workgroup live through its turns"""
    m = _mfx()
    _one_window(monkeypatch)
    k = 31
    rng = np.random.default_rng(701)
    special = np.array([1, 3, 4, 5, 15, 16, 17, 2047, 2048, 2049, 9999, 10000, 10001, 2**22, 2**32 - 1], dtype=np.uint32)
    world = [(k_, np.where(rng.random(len(k_)) < 0.5, rng.integers(1, 40, size=len(k_)), rng.choice(special, size=len(k_))).astype(np.uint32))
             for k_, _ in _trio_world(k)]
    mat, pat, child = world
    positions = sum(len(x[0]) for x in world)
    assert positions > 2 * SCAN_ROUND * TILE
    assert positions > 2 * (cus * 4) * HIST_WG, cus                # every workgroup of the histogram launch: a third turn
    assert len(mat[0]) + len(pat[0]) > 2 * (cus * 4) * HIST_WG     # ... without the child too
    pm, pp, pc = tt._files(m, tmp_path, k, mat, pat, child, "h")
    max_mult = 10000
    _, _, want, wst = tr.reference(mat, pat, child, 1, 1, 1, max_mult)
    assert want[:, 2047].all() and want[:, 2048].all() and want[:, 10000].all()      # both sides of the LDS bound, and the overflow column
    names = ("n_mat", "n_pat", "n_child", "n_both", "n_mat_only", "n_pat_only")
    for agg in (None, "1"):
        if agg:
            monkeypatch.setenv("MFX_SPECTRUM_AGG", agg)
        img, st = m.db_trio_hist(pm, pp, pc, max_mult=max_mult, with_stats=True)
        assert (img == want).all() and int(img[2].sum()) == len(child[0]), (agg, np.argwhere(img != want)[:8])
        assert {n: st[n] for n in names} == {n: wst[n] for n in names} and st["windows"] == 1
        assert (m.db_trio_hist(pm, pp, pc, max_mult=max_mult) == img).all()      # a second run
        img2 = m.db_trio_hist(pm, pp, None, max_mult=max_mult)
        assert (img2[:2] == want[:2]).all() and not img2[2].any()
        for p, d in ((pm, mat), (pp, pat), (pc, child)):
            row, n = m.db_histogram(p, max_mult=max_mult, with_count=True)
            assert n == len(d[0]) and (row == np.bincount(np.minimum(d[1], max_mult).astype(np.int64), minlength=max_mult + 1).astype(np.uint64)).all(), agg


# ---------------------------------------------------------------------------------------------------------------------------------------
# join
# ---------------------------------------------------------------------------------------------------------------------------------------
def _join_sizes(cus, tile):
    """each side's size: together a little more than CUs x 4 tiles and three"""
    return (cus * 4 * tile + 3 * tile) // 2 + 352


def test_join_second_and_third_turns(tmp_path, monkeypatch, cus):
    m = _mfx()
    _one_window(monkeypatch)
    k = 21
    per, tile = m.db_join_grain()
    assert tile == TILE
    n = _join_sizes(cus, tile)
    read, asm = tj._pair(k, "interleaved", n, n, seed=60)
    total = len(read[0]) + len(asm[0])
    tiles = (total + tile - 1) // tile
    assert total > cus * 4 * tile + 3 * tile                       # -completeness (CUs x 4 workgroups): a second turn ...
    assert cus * 4 < tiles < 2 * cus * 4                           # ... in some workgroups only
    assert tiles > 2 * cus * 2                                     # -spectrum (CUs x 2 workgroups): a third turn
    rp, ap = str(tmp_path / "r.mfxk"), str(tmp_path / "a.mfxk")
    m.db_write_flat(rp, k, read[0], read[1])
    m.db_write_flat(ap, k, asm[0], asm[1])
    t, u, img, st = tj.check_paths(m, k, rp, ap, read, asm, table=False, prob=None, tag="big")
    assert st["windows"] == 1
    # readK is an integer and the sums (== the oracle's, asserted above) stay below 2^53: the fp64 adds are exact in any order
    assert (t == np.floor(t)).all() and (u == np.floor(u)).all() and 0 < t.sum() < 2.0**53 and 0 < u.sum() < 2.0**53


def test_join_with_prob_spectrum_second_turn(tmp_path, monkeypatch, cus):
    """the -prob table on a world half the size: the spectrum launch (CUs x 2 workgroups) still takes a second turn, the completeness
    launch has a tile per workgroup"""
    m = _mfx()
    _one_window(monkeypatch)
    k = 21
    per, tile = m.db_join_grain()
    n = _join_sizes(cus, tile) // 2
    read, asm = tj._pair(k, "interleaved", n, n, seed=61)
    total = len(read[0]) + len(asm[0])
    assert total > cus * 2 * tile                                  # -spectrum: a second turn
    rp, ap = str(tmp_path / "r.mfxk"), str(tmp_path / "a.mfxk")
    m.db_write_flat(rp, k, read[0], read[1])
    m.db_write_flat(ap, k, asm[0], asm[1])
    t, u, img, st = tj.check_paths(m, k, rp, ap, read, asm, table=False, prob=tj.PROB, tag="prob")
    assert st["windows"] == 1 and 0 < t.sum() < 2.0**53 and 0 < u.sum() < 2.0**53
