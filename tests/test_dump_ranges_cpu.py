"""tests/dump_ranges.py on its own, without a GPU: the worlds hold what their docstring says, the grid holds every class
of range, the reference agrees with itself and with the oracle's processDump, and the checker fails on answers that are
each wrong in one small way -- the slips the range arithmetic of the -dump kernels could make (no mutant kernel is ever
run: a mutant of that indexing writes out of bounds)."""
import numpy as np
import pytest

from oracle import plain
from oracle import pyoracle as po
from tests import dump_ranges as dr

TILE, LONG, L = dr.TILE, dr.LONG, dr.L_LONG
WORLDS = [(21, True), (20, True), (21, False), (33, True), (64, False)]
IDS = ["k%d-%s" % (k, "canonical" if c else "forward") for k, c in WORLDS]


def _revcomp(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | ((x & 3) ^ 2)
        x >>= 2
    return r


def _near_and_far(ref, hit):
    """hit: per contig a boolean array over the start positions; (one within k of a seam, one further away)"""
    k, near, far = ref.w.k, False, False
    for c, h in enumerate(hit):
        n = len(ref.w.contigs[c])
        for p in np.flatnonzero(h).tolist():
            if dr.seam_distance(p, n) < k:
                near = True
            else:
                far = True
    return near, far


@pytest.mark.parametrize("k,canonical", WORLDS, ids=IDS)
def test_world_holds_what_its_docstring_says(k, canonical):
    w = dr.world(k, canonical)
    ref = dr.Reference(w)
    assert [len(c) for c in w.contigs] == [0, k - 1, k, k + 1, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1, 3 * 4096 + 300]
    c = w.contigs[LONG]
    # every N where stated, and nowhere else
    ns = set(dr.single_ns(k)) | set(range(*dr.N_RUN))
    assert ns == {i for i, ch in enumerate(c) if ch in b"Nn"}
    assert dr.single_ns(k) == [4095, 4096, 8191 - (k - 1), L - k] and dr.N_RUN[0] < 2 * TILE < dr.N_RUN[1]
    assert not any(ch in b"Nn" for x in w.contigs[:LONG] for ch in x)
    lo = {i for i, ch in enumerate(c) if ch in b"acgtn"}
    assert lo == set(range(*dr.LOWER)) and dr.LOWER[0] < TILE < dr.LOWER[1]
    # the tables: the assembly's true counts, by the oracles' own counters
    if canonical and k <= 31:
        ak, av = po.count_kmers(k, w.contigs)
        wk, wv = w.arrays(w.asm)
        assert np.array_equal(ak, wk) and np.array_equal(av, wv)
    elif canonical:
        assert plain.count_kmers(k, [x.decode() for x in w.contigs]) == w.asm
    elif k <= 31:
        fw = {}
        for x in w.contigs:
            for _, f, _r in po.kiter(k, x):
                fw[f] = fw.get(f, 0) + 1
        assert fw == w.asm
    else:
        fw = {}
        for x in w.contigs:
            for _, s in plain.valid_kmers(x.decode(), k):
                fw[plain.enc(s)] = fw.get(plain.enc(s), 0) + 1
        assert fw == w.asm
    if canonical:
        assert all(x <= _revcomp(x, k) for t in (w.read, w.asm) for x in t)
    else:
        # really not canonical: k-mers above their reverse complement are stored, and positions of the contigs answer from them
        assert sum(1 for x in w.asm if x > _revcomp(x, k)) > len(w.asm) // 3
        up = [p for p, f, r in dr.kmers(c, k) if f > r and w.read.get(f, 0) and r not in w.read]
        assert len(up) > 1000 and all(int(ref.rv[LONG][p]) == w.read[f] for p, f, r in dr.kmers(c, k) if p in set(up[:50]))
    # a valid k-mer starts exactly where k bases without an N follow
    for ci, x in enumerate(w.contigs):
        ok = np.array([i + k <= len(x) and not any(ch in b"Nn" for ch in x[i:i + k]) for i in range(len(x))], dtype=bool)
        assert np.array_equal(ok, ref.valid[ci])
    assert not ref.valid[LONG][L - 2 * k + 1:].any() and ref.valid[LONG][L - 2 * k] and not ref.valid[LONG][TILE - k:TILE + 1].any()
    # every special read count within k of a seam and away from one; so the missing k-mers
    for v in dr.SPECIAL:
        assert _near_and_far(ref, [(r == v) & ok for r, ok in zip(ref.rv, ref.valid)]) == (True, True), v
        assert len(w.placed[v]) >= 4 and all(int(ref.rv[ci][p]) == v for ci, p in w.placed[v])
    assert _near_and_far(ref, [(r == 0) & ok for r, ok in zip(ref.rv, ref.valid)]) == (True, True)
    assert sum(1 for v in dr.SPECIAL if v < dr.PEAK / 2) == 5 and 0 < ref.counters(LONG, 0, L)[1] < ref.counters(LONG, 0, L)[0] // 10
    # the tandem repeat: asmV > readK on both sides of the seam at 3 * TILE
    t0, t1 = w.tandem
    assert t0 + k < 3 * TILE < t1 - 2 * k
    for side in (range(3 * TILE - k, 3 * TILE), range(3 * TILE, 3 * TILE + k)):
        for p in side:
            assert ref.valid[LONG][p] and ref.rv[LONG][p] in (dr.TANDEM_READ, 2 * dr.TANDEM_READ)
            assert ref.av[LONG][p] > plain.getK(dr.PEAK, [], [], int(ref.rv[LONG][p]), 0)[0]
    if k <= 31 and k % 2:
        for a in (15, 16):                                     # the two sides of the text writer's table
            assert _near_and_far(ref, [x == a for x in ref.av]) == (True, True), a
    # even k: own-reverse-complement k-mers at ordinary positions and across a seam, answered twice
    if k % 2 == 0:
        assert len(w.palindromes) >= 5
        across = [(ci, p) for ci, p in w.palindromes if any(p < s < p + k for s in dr.seams(len(w.contigs[ci])))]
        assert {ci for ci, _ in across} == {8, LONG} and any(dr.seam_distance(p, L) >= k for ci, p in w.palindromes if ci == LONG)
        for ci, p in w.palindromes:
            f, r = next((f, r) for q, f, r in dr.kmers(w.contigs[ci][p:p + k], k))
            assert f == r and ref.valid[ci][p]
            assert int(ref.rv[ci][p]) == (2 * w.read.get(f, 0)) & 0xffffffff and int(ref.av[ci][p]) == 2 * w.asm[f]
        assert any(ref.rv[ci][p] > 0 for ci, p in across)
    else:
        assert not w.palindromes


@pytest.mark.parametrize("k", [20, 21, 33, 64])
def test_grid_holds_every_class_of_range(k):
    w = dr.world(k)
    ref = dr.Reference(w)
    m = dr.marks(k)
    for x in (0, 1, k - 2, k - 1, k, 255, 256, 257, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1, 8191, 8192, 8193,
              L - k - 1, L - k, L - k + 1, L - k + 2, L - 1, L):
        assert x in m
    for n in dr.single_ns(k):                                  # the first position behind each single N, and + (k - 1)
        assert n + 1 in m and min(n + k, L) in m
    g = dr.grid(w, LONG)
    assert len(g) == len(m) * (len(m) + 1) // 2 and len(set(g)) == len(g) and all(0 <= b <= e <= L for b, e in g)
    assert any(b == e for b, e in g)                                               # an empty range
    assert any(b and b % TILE == 0 and e > b for b, e in g)                        # tile-aligned begin other than 0
    assert any(b % TILE and e > b for b, e in g)                                   # begin inside a tile
    assert any(b % TILE and e > b and b // TILE != (e - 1) // TILE for b, e in g)  # ... and the range goes on into the next
    assert any(L - k + 1 < e < L and b < L - k for b, e in g)                      # end inside the last k - 1 positions
    assert any(e > b and ref.counters(LONG, b, e)[0] == 0 for b, e in g)           # a range with no k-mer at all
    assert any(b - 1 in dr.single_ns(k) and e > b for b, e in g)                   # begin right behind an N
    for c in range(LONG):
        n = len(w.contigs[c])
        want = {r for r in ((0, 0), (0, n), (n, n), (0, 1), (1, n), (n - k + 1, n)) if 0 <= r[0] <= r[1] <= n}
        assert set(dr.grid(w, c)) == want and len(dr.grid(w, c)) == len(want)
    assert dr.grid(w, 0) == [(0, 0)] and (k - 1 - k + 1, k - 1) in dr.grid(w, 1) and (1, k) in dr.grid(w, 2)
    assert dr.grid_size(w) == len(g) + sum(len(dr.grid(w, c)) for c in range(LONG)) > 300


@pytest.mark.parametrize("k,canonical,use_prob", [(21, True, False), (21, True, True), (20, True, False), (21, False, True)])
def test_reference_agrees_with_itself_and_with_process_dump(k, canonical, use_prob):
    w = dr.world(k, canonical)
    K, P = dr.golden_table() if use_prob else (None, None)
    ref = dr.Reference(w, dr.PEAK, K, P)
    p = po.Params(k, dr.PEAK, K, P)
    R, A = po.Lookup(k, *w.arrays(w.read)), po.Lookup(k, *w.arrays(w.asm))
    for c, x in enumerate(w.contigs):
        n = len(x)
        rk, ak, km, kasm, kmis = po.process_dump(p, R, A, x)
        assert ref.counters(c, 0, n) == (kasm, kmis)
        assert np.array_equal(ak[:n], ref.av[c].astype(np.float64))
        want_rk = np.array([po.getK_values(p, int(v), 0)[0] for v in ref.rv[c].tolist()])
        assert np.array_equal(rk[:n], want_rk)
        assert np.array_equal(ref.missing[c], ref.valid[c] & (rk[:n] == 0))
        ends = dr.marks(k) if c == LONG else sorted({y for r in dr.grid(w, c) for y in r})
        for a in ends:
            for b in ends:
                if a <= b:
                    assert ref.counters(c, a, b) == (int(ref.valid[c][a:b].sum()), int(ref.missing[c][a:b].sum()))
                    s = [ref.counters(c, 0, a), ref.counters(c, a, b), ref.counters(c, b, n)]
                    assert (sum(t[0] for t in s), sum(t[1] for t in s)) == (kasm, kmis)
    whole = ref.counters(LONG, 0, L)
    by_zero = int((ref.valid[LONG] & (ref.rv[LONG] == 0)).sum())
    assert (whole[1] > by_zero) if use_prob else (whole[1] == by_zero)      # the table's rows with probK = 0: non-zero counts are missing


def test_reference_of_the_wide_worlds_counts_what_the_window_rule_counts():
    for k, canonical in ((33, True), (64, False)):
        w = dr.world(k, canonical)
        ref = dr.Reference(w)
        for c, x in enumerate(w.contigs):
            starts = [p for p, _f, _r in dr.kmers(x, k)]
            assert ref.counters(c, 0, len(x))[0] == len(starts) and np.array_equal(np.flatnonzero(ref.valid[c]), np.array(starts, dtype=np.int64))


# ---------------------------------------------------------------------------
# the checker can fail
# ---------------------------------------------------------------------------
def _prob_ref():
    return dr.Reference(dr.world(21), dr.PEAK, *dr.golden_table())


def test_checker_accepts_the_reference_and_counts_the_grid():
    ref = _prob_ref()
    assert ref.run_grid(ref.answer) == dr.grid_size(ref.w)
    assert len(ref.partitions[LONG]) == len(dr.grid(ref.w, LONG))
    short = dr.Reference(dr.world(21))
    for b, e in dr.grid(short.w, LONG)[:-1]:                   # one range of the grid never asked for
        short.check(short.answer(LONG, b, e), LONG, b, e)
    with pytest.raises(AssertionError):
        short.assert_grid_done()


def _shifted(ref, b, e):                    # the arrays one position late: readV[i] holds position b + i + 1
    return (ref.rv[LONG][b + 1:e + 1].copy(), ref.av[LONG][b + 1:e + 1].copy()) + ref.counters(LONG, b, e)


def _one_early(ref, b, e):                  # everything of [b - 1, e - 1)
    return ref.answer(LONG, b - 1, e - 1)


def _counted_from_tile(ref, b, e):          # the counters of [tb, e): `gp >= skip` forgotten where they are counted
    rv, av, _, _ = ref.answer(LONG, b, e)
    return (rv, av) + ref.counters(LONG, b // TILE * TILE, e)


def _missing_by_count(ref, b, e):           # kmissing as readV == 0, not readK == 0
    rv, av, ka, _ = ref.answer(LONG, b, e)
    return rv, av, ka, int((ref.valid[LONG][b:e] & (rv == 0)).sum())


def _tail_written(ref, b, e):               # values for starts in the last k - 1 positions (`gp < clen_left` taken for the test)
    rv, av, ka, km = ref.answer(LONG, b, e)
    k = ref.w.k
    for p in range(max(b, L - k + 1), e):
        rv[p - b], av[p - b] = 7, 1
    return rv, av, ka, km


def _tail_counted(ref, b, e):               # ... and counted
    rv, av, ka, km = _tail_written(ref, b, e)
    return rv, av, ka + (e - max(b, L - ref.w.k + 1)), km


def _one_short(ref, b, e):
    rv, av, ka, km = ref.answer(LONG, b, e)
    return rv[:-1], av[:-1], ka, km


K21 = 21
MUTANTS = [
    (_shifted, 4096, 8192), (_shifted, 4097, 4096 + K21), (_shifted, 0, 1),
    (_one_early, 4096, 8192), (_one_early, 4097, L), (_one_early, 1, K21),
    (_counted_from_tile, 4096 + K21 - 1, 8191), (_counted_from_tile, L - K21 - 1, L - 1), (_counted_from_tile, 257, 4095),
    (_missing_by_count, 0, L), (_missing_by_count, 256, 4096 + K21),
    (_tail_written, L - K21 - 1, L), (_tail_written, 8192, L - 1), (_tail_written, L - K21 + 1, L - K21 + 2),
    (_tail_counted, 0, L), (_one_short, 4096, 8192),
]


@pytest.mark.parametrize("mutant,b,e", MUTANTS, ids=["%s-%d-%d" % (f.__name__.strip("_"), b, e) for f, b, e in MUTANTS])
def test_checker_rejects_an_answer_that_is_wrong_in_one_way(mutant, b, e):
    ref = _prob_ref()
    assert (b, e) in dr.grid(ref.w, LONG)
    ref.check(ref.answer(LONG, b, e), LONG, b, e)              # the right answer passes
    with pytest.raises(AssertionError):
        ref.check(mutant(ref, b, e), LONG, b, e)


def test_missing_by_count_is_the_peak_rules_own_answer():
    """without a table readK == 0 exactly where readV == 0 (merfin-globals.C:84-89): that slip shows only under a table, which
    is why the routes that count kmissing on their own (the sharded recount) run the grid with the golden table"""
    ref = dr.Reference(dr.world(21))
    ref.check(_missing_by_count(ref, 0, L), LONG, 0, L)


def test_text_world_is_what_the_chunk_sweep_needs():
    k = 21
    w = dr.text_world(k)
    assert [len(c) for c in w.contigs] == [0, 1, k - 1, k, 4096, 4097, 20011] and w.contigs[6][:L] == dr.world(k).contigs[LONG]
    ak, av = po.count_kmers(k, w.contigs)
    wk, wv = w.arrays(w.asm)
    assert np.array_equal(ak, wk) and np.array_equal(av, wv) and set(w.read) <= set(w.asm)
    # both sides of the text writer's table of tails (read count < 256, assembly count < 16) and the table rows with readK = 0
    assert {1, 8, 9, 255, 256, 60000, 2**22 - 1, 2**32 - 1} <= set(w.read.values()) and {15, 16} <= set(w.asm.values())
