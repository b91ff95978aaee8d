"""Worlds, reference and checker of the -dump range tests (tests/test_dump_ranges_cpu.py, tests/test_gpu_dump_ranges.py,
tests/test_gpu_dump_chunks.py).  A plain module: no fixtures, no GPU.

mfx_dump_values answers for any range [b, e) of a contig, and the text writer asks for one range per chunk; the kernels
start at the tile boundary below b (tb = b / TILE * TILE), skip b - tb positions and store at gp - skip.  What can go wrong
there shows only for ranges that begin or end in particular places, so every route is asked for the same GRID of ranges
and every answer is compared with a reference that no device code wrote.

REFERENCE.  Per contig and start position the pair (readV, asmV) = value(fmer) + value(rmer) in uint32 arithmetic in
both tables (merfin-globals.C:107-108), (0, 0) where no valid k-mer starts: oracle.pyoracle (kiter + Lookup) at k <= 31,
oracle.plain.py_dump at k > 31.  The counters of a range [b, e) are defined here:
    kasm     is the number of positions in [b, e) where a valid k-mer starts;
    kmissing is those of them whose readK == 0 by the oracle's getK (getK_values / plain.getK).
(Under the peak rule every non-zero count gives readK >= 1 -- a count under the peak gives 1, merfin-globals.C:86 -- so
readK == 0 there means readV == 0; with the golden example_lookup_table.txt the rows of the counts 1 ... 8 hold probK = 0 and
a non-zero count is missing.  The low counts are in every world; what they mean depends on the parameters.)

WORLDS.  world(k, canonical): TILE = 4096, PEAK = 26.  Contigs, in this order, of the lengths 0, k - 1, k, k + 1, 4095,
4096, 4097, 4096 + k - 2, 4096 + k - 1 and L = 3 * 4096 + 300 (the LONG contig, index LONG).  On the long contig:
  - single Ns at 4095, 4096, 8191 - (k - 1) and L - k;
  - an N run [8189, 8195) across the seam at 8192;
  - a lower-case stretch [4046, 4146) across the seam at 4096;
  - a tandem repeat that begins 110 positions before the seam at 12288 and ends behind it: unit of 11 bases (odd k) or a
    unit w + revcomp(w) of k bases (even k: the k-mers of phase 0 and k / 2 are their own reverse complement, one of them
    lies across the seam); 16 copies at k <= 31 -- its k-mers occur 15 or 16 times, the two sides of the text writer's
    table --, 24 or 4 copies at k > 31 (odd, even).  Its k-mers get the read count 52 (readK 2 < asmV) on both sides of the seam.
  - even k: further own-reverse-complement k-mers at 1500 and 2500, and one across the seam of the contig of length
    4096 + k - 1 (start 4096 - k / 2).
The assembly counts are the true counts of the contigs' k-mers (what a sequence-only index counts for itself).  The read
count of a k-mer is about PEAK times its assembly count, 0 for a few per cent of them; a few hundred read k-mers are in no
contig.  SPECIAL read counts -- 1, 3, 8 (under PEAK / 2, table rows with probK = 0), 9, 12 (under PEAK / 2, rows with probK
= 1), 255 / 256 (the text writer's table ends at 255), 60000, 2**22 - 1, 2**32 - 1 (the compact layout's side table) -- sit
on k-mers that start within k of a seam (behind the seams at 4096 and 8192 of the long contig, across the seam of the
contig of length 4096 + k - 1) and at ordinary positions of the long contig (300 + 37 i).  world.placed lists them.
canonical = False: the tables hold the forward k-mers of the contigs as they are (both strands are probed and summed).

GRID.  grid(world, c): on the long contig all pairs begin <= end of the marks 0, 1, k - 2, k - 1, k, 255, 256, 257, 4095,
4096, 4097, 4096 + k - 2, 4096 + k - 1, 8191, 8192, 8193, L - k - 1, L - k, L - k + 1, L - k + 2, L - 1, L, the first position
behind each single N and that position + (k - 1); on every other contig (0, 0), (0, len), (len, len), (0, 1), (1, len),
(len - k + 1, len) where they exist.
"""
import functools
import os

import numpy as np

from oracle import plain
from oracle import pyoracle as po
from tests import synth

TILE = 4096
PEAK = 26.0
L_LONG = 3 * TILE + 300
LONG = 9                                            # index of the long contig
N_RUN = (8189, 8195)
LOWER = (4046, 4146)
SPECIAL = (1, 3, 8, 9, 12, 255, 256, 60000, 2**22 - 1, 2**32 - 1)
TANDEM_READ = 52
GOLDEN_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example_lookup_table.txt")

_CODE = {}
for _ch, _c in zip("ACTG", range(4)):               # meryl's 2-bit codes; the complement is code ^ 2
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _c


def contig_lengths(k):
    return [0, k - 1, k, k + 1, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1, L_LONG]


def single_ns(k):
    return [4095, 4096, 8191 - (k - 1), L_LONG - k]


def seams(n):
    return list(range(TILE, n + 1, TILE))


def seam_distance(p, n):
    """distance of start position p to the nearest tile seam inside a contig of n positions (n itself where there is none)"""
    return min([abs(p - s) for s in seams(n)] or [n])


def kmers(contig, k):
    """(start, fmer, rmer) of every valid k-mer of a contig (bytes), as Python integers: any k.  Only the worlds are
    built with it; the CPU tests hold the tables it makes against the oracles' counters."""
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    f = r = run = 0
    for i, ch in enumerate(contig):
        c = _CODE.get(ch)
        if c is None:
            run = 0
            continue
        f = ((f << 2) | c) & mask
        r = (r >> 2) | ((c ^ 2) << top)
        run += 1
        if run >= k:
            yield i - k + 1, f, r


def _revcomp_bytes(a):
    comp = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}
    return np.array([comp[int(x)] for x in a[::-1]], dtype=np.uint8)


def to_rows(ints):
    a = np.zeros((len(ints), 2), dtype=np.uint64)
    for i, x in enumerate(ints):
        a[i, 0] = x & 0xffffffffffffffff
        a[i, 1] = x >> 64
    return a


class World:
    """contigs (bytes), read / asm {k-mer as int: count}, tandem (begin, end) on the long contig, placed {special count:
    [(contig, start)]}, palindromes [(contig, start)]"""

    def __init__(self, k, canonical, contigs, read, asm, tandem, placed, palindromes):
        self.k, self.canonical, self.contigs, self.read, self.asm = k, canonical, contigs, read, asm
        self.tandem, self.placed, self.palindromes = tandem, placed, palindromes

    def arrays(self, table):
        """(k-mers, counts) of self.read or self.asm as the library and the C oracle take them: k-mers ascending, uint64 at
        k <= 31, rows {low, high} beyond"""
        keys = sorted(table)
        vals = np.array([table[x] for x in keys], dtype=np.uint32)
        return (to_rows(keys) if self.k > 31 else np.array(keys, dtype=np.uint64)), vals


@functools.lru_cache(maxsize=None)
def world(k, canonical=True):
    r = synth.rng(7000 + 2 * k + (0 if canonical else 1))
    lens = contig_lengths(k)
    cs = [synth.random_contig(r, n) for n in lens]
    c = cs[LONG]
    palindromes = []
    # the tandem repeat across the seam at 3 * TILE
    copies = 16 if k <= 31 else (24 if k % 2 else 4)
    if k % 2:
        unit, extra = synth.random_contig(r, 11), 5
    else:
        w = synth.random_contig(r, k // 2)
        unit, extra = np.concatenate([w, _revcomp_bytes(w)]), 10
    t0 = 3 * TILE - 110
    t1 = t0 + len(unit) * (copies - 1) + k + extra
    c[t0:t1] = np.tile(unit, (t1 - t0) // len(unit) + 1)[:t1 - t0]
    if k % 2 == 0:
        palindromes += [(LONG, p) for p in range(t0, t1 - k + 1, k // 2)]
        for at in (1500, 2500):
            w = synth.random_contig(r, k // 2)
            c[at:at + k] = np.concatenate([w, _revcomp_bytes(w)])
            palindromes.append((LONG, at))
        w = synth.random_contig(r, k // 2)
        cs[8][TILE - k // 2:TILE + k // 2] = np.concatenate([w, _revcomp_bytes(w)])
        palindromes.append((8, TILE - k // 2))
    for n in single_ns(k):
        c[n] = ord("N")
    c[N_RUN[0]:N_RUN[1]] = ord("N")
    c[LOWER[0]:LOWER[1]] |= 0x20
    contigs = synth.as_bytes(cs)
    assert [len(x) for x in contigs] == lens and 3 * TILE + 2 * k < t1 < L_LONG - k
    # the k-mers: every occurrence, and the assembly's true counts
    occ = [{p: (f if not canonical else min(f, rr)) for p, f, rr in kmers(x, k)} for x in contigs]
    asm = {}
    for o in occ:
        for x in o.values():
            asm[x] = asm.get(x, 0) + 1
    read = {}
    for x in sorted(asm):
        v = int(PEAK * asm[x]) + int(r.integers(-3, 4))
        if r.random() >= 0.04:
            read[x] = v
    for p in range(t0, t1 - k + 1):
        read[occ[LONG][p]] = TANDEM_READ
    # special counts near the seams and at ordinary positions
    near = [(LONG, p) for p in range(TILE + 1, TILE + k)] + [(LONG, p) for p in range(N_RUN[1], 2 * TILE + k)]
    near += [(8, p) for p in range(TILE - k + 1, TILE)]
    far = [(LONG, 300 + 37 * i) for i in range(2 * len(SPECIAL))]
    pal = set(palindromes)
    near = [(ci, p) for ci, p in near if p in occ[ci] and not any((ci, q) in pal for q in range(p - k, p + k))]
    assert len(near) >= 2 * len(SPECIAL) and all(p in occ[ci] for ci, p in far)
    placed = {}
    for spots in (near, far):
        for i, (ci, p) in enumerate(spots):
            v = SPECIAL[i % len(SPECIAL)]
            read[occ[ci][p]] = v
            placed.setdefault(v, []).append((ci, p))
    # read k-mers that are in no contig
    for _ in range(300):
        w = synth.random_contig(r, k).tobytes()
        _, f, rr = next(kmers(w, k))
        x = min(f, rr) if canonical else f
        if x not in asm:
            read[x] = int(r.integers(1, 4))
    return World(k, canonical, contigs, read, asm, (t0, t1), placed, palindromes)


@functools.lru_cache(maxsize=None)
def text_world(k=21):
    """the world of the text writer's tests (tests/test_gpu_dump_chunks.py): contigs of 0, 1, k - 1, k, 4096, 4097 and 20011
    positions; the last one begins with the long contig of world(k) -- its Ns, its repeat, its special counts keep their
    positions -- and goes on with random bases.  Assembly counts: the true counts; read counts: world(k)'s where it has the
    k-mer, about PEAK times the assembly count otherwise"""
    w = world(k)
    r = synth.rng(7700 + k)
    cs = [synth.random_contig(r, n).tobytes() for n in (0, 1, k - 1, k, 4096, 4097)]
    cs.append(w.contigs[LONG] + synth.random_contig(r, 20011 - L_LONG).tobytes())
    asm = {}
    for x in cs:
        for _, f, rr in kmers(x, k):
            asm[min(f, rr)] = asm.get(min(f, rr), 0) + 1
    read = {}
    for x in sorted(asm):
        v = w.read.get(x, 0) if x in w.asm else (int(PEAK * asm[x]) + int(r.integers(-3, 4)) if r.random() >= 0.04 else 0)
        if v:
            read[x] = v
    return World(k, True, cs, read, asm, w.tandem, {}, [])


def marks(k):
    m = [0, 1, k - 2, k - 1, k, 255, 256, 257, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1, 8191, 8192, 8193,
         L_LONG - k - 1, L_LONG - k, L_LONG - k + 1, L_LONG - k + 2, L_LONG - 1, L_LONG]
    for n in single_ns(k):
        m += [n + 1, min(n + 1 + (k - 1), L_LONG)]
    return sorted(set(m))


def grid(w, c):
    n = len(w.contigs[c])
    if c == LONG:
        m = marks(w.k)
        return [(b, e) for b in m for e in m if b <= e]
    g = []
    for b, e in ((0, 0), (0, n), (n, n), (0, 1), (1, n), (n - w.k + 1, n)):
        if 0 <= b <= e <= n and (b, e) not in g:
            g.append((b, e))
    return g


def grid_size(w):
    return sum(len(grid(w, c)) for c in range(len(w.contigs)))


@functools.lru_cache(maxsize=None)
def _values(k, canonical):
    """[(readV, asmV, valid)] per contig of world(k, canonical), from the oracles; at k > 31 also plain's readK (peak rule)"""
    w = world(k, canonical)
    out = []
    if k <= 31:
        R, A = po.Lookup(k, *w.arrays(w.read)), po.Lookup(k, *w.arrays(w.asm))
        for c in w.contigs:
            rv, av, ok = np.zeros(len(c), np.uint32), np.zeros(len(c), np.uint32), np.zeros(len(c), bool)
            for p, f, r in po.kiter(k, c):
                rv[p] = (R.value(f) + R.value(r)) & 0xffffffff
                av[p] = (A.value(f) + A.value(r)) & 0xffffffff
                ok[p] = True
            out.append((rv, av, ok))
    else:
        for c in w.contigs:
            rv, av, ok = np.zeros(len(c), np.uint32), np.zeros(len(c), np.uint32), np.zeros(len(c), bool)
            for p, v in plain.py_dump(k, PEAK, [], [], c.decode(), w.read, w.asm).items():
                rv[p], av[p], ok[p] = v[0], v[1], True
            out.append((rv, av, ok))
    return out


class Reference:
    """the reference of one world under one set of K* parameters, and the checker of the answers to it"""

    def __init__(self, w, peak=PEAK, probK=None, probP=None):
        self.w, self.peak = w, peak
        self.probK = [] if probK is None else [int(x) for x in probK]
        self.probP = [] if probP is None else [float(x) for x in probP]
        self.rv, self.av, self.valid, self.missing = [], [], [], []
        p = po.Params(w.k, peak, self.probK or None, self.probP or None) if w.k <= 31 else None
        for rv, av, ok in _values(w.k, w.canonical):
            if p is not None:
                zero = {int(v): po.getK_values(p, int(v), 0)[0] == 0 for v in np.unique(rv).tolist()}
            else:
                zero = {int(v): plain.getK(peak, self.probK, self.probP, int(v), 0)[0] == 0 for v in np.unique(rv).tolist()}
            mis = ok & np.array([zero[int(v)] for v in rv.tolist()], dtype=bool)
            self.rv.append(rv)
            self.av.append(av)
            self.valid.append(ok)
            self.missing.append(mis)
        self._cv = [np.concatenate([[0], np.cumsum(x)]) for x in self.valid]
        self._cm = [np.concatenate([[0], np.cumsum(x)]) for x in self.missing]
        self.seen = [dict() for _ in w.contigs]        # contig -> {(b, e): (kasm, kmissing) as answered}
        self.partitions = [set() for _ in w.contigs]    # contig -> {(x, y)}: answers of (0, x), (x, y), (y, len) added up

    def counters(self, c, b, e):
        return int(self._cv[c][e] - self._cv[c][b]), int(self._cm[c][e] - self._cm[c][b])

    def answer(self, c, b, e):
        """what a correct route returns for [b, e) of contig c"""
        return (self.rv[c][b:e].copy(), self.av[c][b:e].copy()) + self.counters(c, b, e)

    def check(self, got, c, b, e):
        """got = (readV, asmV, kasm, kmissing) as answered for [b, e) of contig c: lengths, arrays, counters, and -- with
        the answers checked before -- every three-way partition (0, x), (x, y), (y, len) of the contig that this range
        completes adds up to the answer for the whole contig"""
        rv, av, ka, km = got
        at = "contig %d [%d, %d)" % (c, b, e)
        assert len(rv) == e - b and len(av) == e - b, at
        if e > b:
            bad = np.flatnonzero((np.asarray(rv) != self.rv[c][b:e]) | (np.asarray(av) != self.av[c][b:e]))
            assert len(bad) == 0, "%s: %d positions differ, the first at %d: got (%d, %d), want (%d, %d)" % (
                at, len(bad), b + bad[0], rv[bad[0]], av[bad[0]], self.rv[c][b + bad[0]], self.av[c][b + bad[0]])
        assert (int(ka), int(km)) == self.counters(c, b, e), at
        seen, n = self.seen[c], len(self.w.contigs[c])
        seen[(b, e)] = (int(ka), int(km))
        if (0, n) not in seen:
            return
        ends = sorted({x for r in seen for x in r})
        cand = [(b, e)] if (b, e) != (0, n) else []
        if b == 0:
            cand += [(e, y) for y in ends if y >= e]
        if e == n:
            cand += [(x, b) for x in ends if x <= b]
        if (b, e) == (0, n):
            cand = [(x, y) for x in ends for y in ends if x <= y]
        for x, y in cand:
            if (0, x) in seen and (x, y) in seen and (y, n) in seen:
                s = tuple(seen[(0, x)][i] + seen[(x, y)][i] + seen[(y, n)][i] for i in (0, 1))
                assert s == seen[(0, n)], "%s: the answers for (0, %d), (%d, %d), (%d, %d) add up to %s, the contig's is %s" % (at, x, x, y, y, n, s, seen[(0, n)])
                self.partitions[c].add((x, y))

    def assert_grid_done(self):
        """every range of the grid was checked, and every three-way partition the grid holds was added up"""
        for c in range(len(self.w.contigs)):
            g, n = set(grid(self.w, c)), len(self.w.contigs[c])
            assert g <= set(self.seen[c]), (c, sorted(g - set(self.seen[c]))[:5])
            want = {(x, y) for (x, y) in g if (0, x) in g and (y, n) in g}
            assert want <= self.partitions[c], (c, sorted(want - self.partitions[c])[:5])

    def run_grid(self, fn):
        """fn(contig, begin, end) -> (readV, asmV, kasm, kmissing) over the whole grid; returns the number of ranges"""
        n = 0
        for c in range(len(self.w.contigs)):
            for b, e in grid(self.w, c):
                self.check(fn(c, b, e), c, b, e)
                n += 1
        self.assert_grid_done()
        return n


def golden_table():
    return po.load_kmetric(GOLDEN_TABLE)


def name_of(c):
    return "ctg%d" % c


def dump_text(w, path, probK=None, probP=None, contigs=None, peak=PEAK):
    """the oracle's -dump text (process_dump + output_dump) of the given contigs (default: all) one after another, k <= 31:
    (bytes, {contig: (kasm, kmissing)})"""
    p = po.Params(w.k, peak, probK, probP)
    R, A = po.Lookup(w.k, *w.arrays(w.read)), po.Lookup(w.k, *w.arrays(w.asm))
    counters = {}
    open(path, "wb").close()
    for c in (range(len(w.contigs)) if contigs is None else contigs):
        rk, ak, km, kasm, kmis = po.process_dump(p, R, A, w.contigs[c])
        po.output_dump(path, name_of(c), rk, ak, km, append=True)
        counters[c] = (kasm, kmis)
    with open(path, "rb") as f:
        return f.read(), counters
