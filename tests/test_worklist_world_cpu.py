"""The worlds of tests/worklist_world.py hold what tests/test_gpu_worklist.py needs -- asserted from the oracle alone, so that a change of
the recipe that loses a class fails here, without a device."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import worklist_world as ww


@pytest.fixture(scope="module", params=ww.KS, ids=["k%d" % k for k in ww.KS])
def w(request):
    return ww.world(request.param)


def test_shape_of_the_world(w):
    assert sum(len(c) for c in w.contigs) <= 300000 and len(w.contigs) == 3
    assert all(len(c) % ww.TILE for c in w.contigs)
    assert any(b"N" * 50 in c for c in w.contigs) and any(any(97 <= b <= 116 for b in c[:20000]) for c in w.contigs)
    assert w.ntiles == sum((len(c) + ww.TILE - 1) // ww.TILE for c in w.contigs)
    assert len(w.planted) >= ww.N_SAT and set(np.unique(w.read[1][np.isin(w.read[0], w.planted)]).tolist()) == set(ww.SAT_VALUES)


def test_host_positions_are_the_oracles_kmers(w):
    """canonical_positions (numpy) against the oracle's counter and iterator: the host side of the list checks rests on it"""
    allk = np.concatenate([km[ok] for km, ok, _ in w.pos])
    u, n = np.unique(allk, return_counts=True)
    np.testing.assert_array_equal(u, w.asm[0])
    np.testing.assert_array_equal(n.astype(np.uint32), w.asm[1])
    c = w.contigs[2]
    km, ok, pal = w.pos[2]
    seen = 0
    for p, f, r in po.kiter(w.k, c):                              # (the iterator's position: the k-mer's first base)
        assert ok[p] and km[p] == min(f, r) and pal[p] == (f == r), p
        seen += 1
    assert seen == int(ok.sum())


def test_saturated_positions_per_contig(w):
    for ci in range(3):
        p = w.positions_in(ci, w.sat)
        tiles, waves = np.unique(w.tile_of(ci, p)), np.unique(w.wave_of(p))
        print("k = %d contig %d: %d saturated positions in %d tiles" % (w.k, ci, len(p), len(tiles)))
        assert len(p) >= 300 and len(tiles) >= 4 and waves.tolist() == [0, 1, 2, 3], (ci, len(p), tiles, waves)
    assert sum(len(w.positions_in(ci, w.sat)) for ci in range(3)) >= ww.N_SAT


def test_saturated_palindromes_at_even_k(w):
    found = []
    for ci, (km, ok, pal) in enumerate(w.pos):
        p = np.nonzero(pal & np.isin(km, w.sat))[0]
        found += [(int(t), int(v)) for t, v in zip(w.tile_of(ci, p), w.wave_of(p))]
        assert w.k % 2 == 0 or not pal.any()
    if w.k % 2:
        assert not found
        return
    assert len(found) >= 40 and len(set(t for t, _ in found)) >= 20 and set(v for _, v in found) == {0, 1, 2, 3}, found
    in_array = [at for ci, at in w.pal_at if ci == 1 and ww.ARRAY_AT <= at < ww.ARRAY_AT + ww.ARRAY_UNIT * ww.ARRAY_COPIES]
    assert len(in_array) >= 4
    for ci, at in w.pal_at:
        assert w.pos[ci][2][at] and w.pos[ci][0][at] in w.sat


def test_filtered_to_missing(w):
    """the saturated k-mers above -max are missing: per contig, in several tiles, and the oracle counts exactly them on top of the unfiltered run"""
    n = 0
    for ci in range(3):
        p = w.positions_in(ci, w.sat_missing)
        assert len(p) >= 20 and len(np.unique(w.tile_of(ci, p))) >= 2, (ci, len(p))
        n += len(p)
    assert n >= 100
    # (no unfiltered oracle run: a read count of 2^32 - 1 is K* bin 1.2e9 there, 10 GB of bins)
    g, _, km, _ = po.hist_run(po.Params(w.k, ww.PEAK), po.Lookup(w.k, w.read[0], w.read[1], 0, ww.READ_MAX), po.Lookup(w.k, *w.asm), w.contigs, threads=4)
    absent, above = w.asm[0][w.asm_read == 0], w.asm[0][w.asm_read > ww.READ_MAX]
    np.testing.assert_array_equal(km, [len(w.positions_in(ci, absent)) + len(w.positions_in(ci, above)) for ci in range(3)])
    assert g.kmissing == int(km.sum()) and sum(len(w.positions_in(ci, above)) for ci in range(3)) >= n


def test_a_wave_with_fewer_than_64_wanted_positions(w):
    """the last tile of the last contig: 300 bases, every k-mer saturated"""
    km, ok, _ = w.pos[2]
    p = np.arange(4 * ww.TILE, len(w.contigs[2]))
    p = p[ok[p]]
    assert len(p) >= 200 and np.isin(km[p], w.sat).all()
    per_wave = np.bincount(((p % ww.BLOCK) // 64) + ww.WAVES * ((p % ww.TILE) // ww.BLOCK))
    assert (per_wave[per_wave > 0] < 64).any() and w.tile_contig(w.ntiles - 1) == 2


def test_far_bins_at_the_second_peak(w):
    """at FAR_PEAK the saturated read counts under the filter fall into K* bins beyond 1024: what take_overflow must return"""
    g = po.hist_run(po.Params(w.k, ww.FAR_PEAK), po.Lookup(w.k, w.read[0], w.read[1], 0, ww.READ_MAX), po.Lookup(w.k, *w.asm), w.contigs, threads=4)[0]
    assert int(np.asarray(g.over())[1024:].sum()) >= 500


@pytest.mark.parametrize("k", [k for k in ww.KS if k <= 30])
def test_minimizers_with_more_kmers_than_two_lines_hold(k):
    """A compact table's line is chosen by the k-mer's minimizer alone (csrc/mfx_place.h: line = (top * nlines) >> 32 with `top` the high
    bits of the placement number), a line has 16 slots: a minimizer with more than 32 k-mers displaces some of them past the home line AND
    the next candidate line at any table size -- the queries the -hist kernel lists as mode 0 / 1.  (The placement number of a 31-mer
    takes 65 bits and has no host entry, mfx_db_place_keys stops at k = 30; k = 31 shares the recipe.)"""
    import merfin_amd as m
    w = ww.world(k)
    P = m.db_place_keys(k, w.asm[0])
    top = P >> np.uint64(max(2 * (k - 3) - 32, 0) + 9)
    _, n = np.unique(top, return_counts=True)
    print("k = %d: largest minimizer %d k-mers, %d minimizers with more than 32" % (k, n.max(), int((n > 32).sum())))
    assert n.max() >= 38 and (n > 32).sum() >= 10


def test_worklist_hooks_refuse_null_arguments():
    """the two test hooks of the list check their arguments before they touch a device"""
    import ctypes as C
    import merfin_amd as m
    L = m.load_library()
    assert L.mfx_eval_debug_worklist(None, 1, 0) != 0 and b"null argument" in L.mfx_last_error()
    n = C.c_uint64(7)
    assert L.mfx_eval_debug_worklist_read(None, 0, None, None, None, 0, None, 0, C.byref(n)) != 0 and b"null argument" in L.mfx_last_error()
