"""An exhaustive (read count, assembly count) grid for the K* evaluation, and an exact reference of -hist over it.

The -hist kernels turn a (readV, asmV) pair into a bin and a koverCpy term through a stack of exact shortcuts (an LDS table
of readK, tabulated bins and terms for small (readK, asmV), three destinations for a bin).  The synthetic worlds of the
other tests keep readK / asmK near 1, so almost none of those tables' entries are ever compared with anything.  Here the
pairs themselves are the input: a candidate set that covers every tabulated entry and both sides of every threshold is
assigned, through a seeded permutation, to the distinct k-mers of a random ~40 kb assembly (`Index.add_read` / `add_asm`
take arbitrary values, and so does the oracle).

What is here is plain Python on IEEE doubles, written from the reference's formulas (merfin-globals.C:66-98,
merfin-histogram.C:54-91) independently of oracle/merfin_oracle.c and of the library:
  * `configs`, `candidates`, `keep`: the K* configurations and the pairs a configuration can hold;
  * `build_world`: contigs and the two tables;
  * `reference`: every bin, kasm, kmissing, the per-contig counters, and koverCpy twice -- `S`, the exact rational sum of
    the double terms, and `F`, the sum of the terms rounded to units of 2^-52 (`kfix`), which is what an integer-summing
    kernel adds up.
No constant of the code under test is written out here: the table sizes arrive as the parameters `maxp`, `klut`, `nb_lds`
and `field` (the caller reads them from the project's headers, tests/test_kstar_grid_cpu.py: project_constants).

A pair is kept only if its bin index is <= BIN_LIMIT and the unconverted bin value is below 2^31: the oracle's (and the
reference program's) arrays are dense up to the largest bin.  asmV == 0 with readK > 0 divides by zero: the bin value is
+inf, which the conversion the reference was compiled with turns into bin 0 (mfx_kstar.h states that rule); those pairs stay.

Recorded figures (tests/test_kstar_grid_cpu.py prints them and asserts the floors; worlds of k = 21, 31, 22, seed 1):

  configuration   candidates  kept    distinct bins >= nb_lds   n_under   oracle koverCpy vs S, relative (worst of three k)
  peak1           36187       36001   1482                       1.8 k    8.1e-16
  peak17.3        37843       37256    431                      11.2 k    1.6e-15
  prob26          37784       37229    422                      15.4 k    3.1e-15
  peak2           37835       37651    707                       3.2 k    9.8e-16
  peak0.75        37400       37208   2179                       2.3 k    1.6e-15
  peak2e-7        27455       21250   1058                       6.1 k    5.7e-15
  prob26-p01      37784       37229    422                      15.4 k    2.9e-15
(the candidates beyond peak1's 36187 are the threshold pairs restated in readK: `readk_preimage`)

Bounds, derived (not measured):
  * oracle, a sequential fp64 sum of n_under non-negative terms: |oracle - S| <= n_under * 2^-53 * S (2e-13 ... 1.7e-12
    relative here: the measured error sits a factor 10^2 ... 10^3 below);
  * integer-sum device routes (mfx_hist_kernel, mfx_hist_rest_kernel):
    |got - S| <= (n_under + (W + 64) * S) * 2^-53, W = (block / 64) * ntiles words -- one rounding to 2^-52 units per term,
    one uint64 -> double conversion per (tile, wave) word, a fixed-order fp64 sum of the words; 1.2e-14 ... 1.3e-14 relative
    at these sizes, against the 1e-12 of the older tests;
  * the sharded route truncates each term to 2^-52 units and converts one integer: |got - S| <= n_under * 2^-52 + S * 2^-53
    (3.6e-16 ... 1.0e-15 relative here);
  * the k > 32 route sums doubles: rel 1e-12 against S, as before.
Measured on an MI355X (tests/test_gpu_kstar_grid.py prints every figure), worst case over the configurations, relative to S:
  k21seq 7.6e-17, k31seq 8.9e-17, k19seq 1.3e-16, k25seq 8.0e-17, k22seq 1.5e-16, k21full 1.1e-16, k11fwd 1.5e-16
  (bound 1.2e-14 ... 1.3e-14); k21shard3 2.0e-16 (bound 1.0e-15 for that configuration); k33wide 1.2e-16 (bar 1e-12).
"""
import math
from collections import Counter
from fractions import Fraction

import numpy as np

from tests import synth

BIN_LIMIT = 200000
U32 = 2 ** 32
SIZES = (4096, 4097, 8191, 500, 20, 0)          # after the first contig, whose length grows until the k-mers suffice


def load_prob(path):
    """-prob table: a line with exactly two ','-separated fields is a row, row n <-> read count n (merfin-globals.C:21-62)"""
    K, P = [], []
    for line in open(path):
        w = [x for x in line.strip().split(",") if x]
        if len(w) == 2:
            K.append(int(w[0]))
            P.append(float(w[1]))
    return K, P


def configs(prob_path):
    """(name, peak, probK, probP).  The last is prob26 with rows of exactly 0.0 and 1.0 (the ends of the range mfx_kfix is
    defined on): rows 10 and 12, whose probK is 1, so that both produce terms."""
    K, P = load_prob(prob_path)
    P01 = list(P)
    assert K[9] == 1 and K[11] == 1
    P01[9], P01[11] = 0.0, 1.0
    return [("peak1", 1.0, [], []), ("peak17.3", 17.3, [], []), ("prob26", 26.0, K, P), ("peak2", 2.0, [], []),
            ("peak0.75", 0.75, [], []), ("peak2e-7", 2e-7, [], []), ("prob26-p01", 26.0, K, P01)]


ORDINARY = ("peak1", "peak17.3", "prob26", "peak2", "peak0.75")      # the five of the issue whose readK table is enabled


# ---------------------------------------------------------------------------
# K* of one pair
# ---------------------------------------------------------------------------
def get_readk(v, peak, probK, probP):
    """(readK, prob) of a read count.  C round() is half away from zero."""
    if v == 0:
        rk = 0.0
    elif v < peak:
        rk = 1.0
    else:
        q = v / peak
        f = math.floor(q)
        rk = float(f + 1) if q - f >= 0.5 else float(f)
    prob = 1.0
    if 0 < v <= len(probK):
        rk, prob = float(probK[v - 1]), float(probP[v - 1])
    return rk, prob


def kfix(t):
    """a term in [0, 1] in units of 2^-52, rounded to nearest even: the bit pattern of t + 1.0 minus that of 1.0"""
    return int(np.float64(t + 1.0).view(np.uint64)) - 0x3FF0000000000000


def evaluate(rv, av, cfg):
    """One pair -> (readK, asmK, prob, kind, bin value, bin, term); kind 'm' missing, 'u' asmK > readK, 'o' otherwise."""
    _, peak, probK, probP = cfg
    rk, prob = get_readk(rv, peak, probK, probP)
    ak = float(av)
    if rk == 0:
        return rk, ak, prob, "m", None, None, None
    under = ak > rk
    hi, lo = (ak, rk) if under else (rk, ak)
    if lo == 0:
        x, idx = math.inf, 0
    else:
        x = ((hi / lo - 1) + 0.1) / 0.2
        idx = int(x) & 0xffffffff if x < 2.0 ** 63 else 0
    term = (1.0 - rk / ak) * prob if under else None
    return rk, ak, prob, ("u" if under else "o"), x, idx, term


def kmetric(rk, ak):
    if rk == 0:
        return 0.0
    if ak > rk:
        return (ak / rk - 1) * -1
    if ak < rk:
        return rk / ak - 1 if ak != 0 else math.inf
    return 0.0


# ---------------------------------------------------------------------------
# candidate pairs
# ---------------------------------------------------------------------------
def candidates(cfg, maxp, klut, nb_lds, field, nbins_list):
    name, peak, probK, probP = cfg
    S = set()
    rows = range(0, maxp + 8)
    cols = range(1, klut + 2)
    if name == "peak2e-7":
        for rv in list(rows) + [field, field + 1, 65536]:
            rk, _ = get_readk(rv, peak, probK, probP)
            for f in (0.25, 0.5, 1, 1.00001, 2, 7.3, 1000, 1 / 1024.0, 1 / 5000.0, 1 / 70000.0, 1 / 300000.0):
                for d in (-1, 0, 1):
                    S.add((rv, min(max(int(rk * f) + d, 0), U32 - 1)))
            S.add((rv, min(max(int(rk / (205 + rv)), 0), U32 - 1)))      # a far `over` bin of its own for every read count
        return sorted(S)
    edge_r = [maxp - 1, maxp, maxp + 1, field - 1, field, field + 1, field + 2, 65535, 65536, 2 ** 31 - 1, 2 ** 31, U32 - 2, U32 - 1]
    small_r = [0, 1, 2, 17, 26, klut - 1, klut, klut + 1, len(probK) or 184, (len(probK) or 184) + 1]
    edge_a = [1, 2, klut - 1, klut, klut + 1, field - 1, field, field + 1, 65535, 65536, 2 ** 31, U32 - 1]
    S.update((r, a) for r in rows for a in cols)
    S.update((r, a) for r in edge_r + small_r for a in edge_a)
    S.update((r, a) for r in edge_r for a in cols)
    S.update((r, 0) for r in (0, 1, 5, 30, 31, 32, 2000, U32 - 1))
    for nbins in nbins_list:
        for T in (nb_lds - 1, nb_lds, nb_lds + 1, nbins - 1, nbins, nbins + 1):
            for lo in list(range(1, 41)) + [1000]:
                for d in (-1, 0, 1, 2):
                    hi = int(math.floor(lo * (0.2 * T + 0.9))) + d
                    S.add((hi, lo))
                    S.add((lo, hi))
                    # the same ratio in readK: a read count whose readK is hi (lo), where this configuration has one -- at
                    # peak 1 these are the two pairs above, elsewhere they are what puts a k-mer on the threshold itself
                    for rk, av in ((hi, lo), (lo, hi)):
                        rv = readk_preimage(rk, cfg)
                        if rv is not None:
                            S.add((rv, av))
    return sorted(S)


def readk_preimage(rk, cfg):
    """a read count whose readK is rk under cfg, or None"""
    _, peak, probK, probP = cfg
    v0 = int(round(rk * peak))
    for v in (v0, v0 - 1, v0 + 1):
        if 0 < v < U32 and get_readk(v, peak, probK, probP)[0] == rk:
            return v
    return None


def keep(cands, cfg):
    out = []
    for rv, av in cands:
        _, _, _, kind, x, idx, _ = evaluate(rv, av, cfg)
        if kind == "m" or x == math.inf or (idx <= BIN_LIMIT and x < 2.0 ** 31):
            out.append((rv, av))
    return out


def thin(pairs, maxp, step=4):
    """every `step`-th readV row plus all edges (the rows from maxp - 1 on and the small edge counts)"""
    small = {0, 1, 2, 17, 26, 31, 32, 33, 184, 185}
    return [(r, a) for r, a in pairs if r % step == 0 or r >= maxp - 1 or r in small or a == 0]


# ---------------------------------------------------------------------------
# k-mers of a contig (meryl's 2-bit code: A 0, C 1, T 2, G 3; the complement is code ^ 2)
# ---------------------------------------------------------------------------
def contig_kmers(contig, k):
    """(n, start positions, forward k-mers, reverse-complement k-mers) of every valid k-mer, the k-mers as Python ints"""
    b = np.frombuffer(contig, dtype=np.uint8) & 0xDF
    n = len(b)
    if n < k:
        return n, [], [], []
    code = np.zeros(n, dtype=np.uint8)
    ok = np.zeros(n, dtype=bool)
    for ch, c in ((65, 0), (67, 1), (84, 2), (71, 3)):
        code[b == ch] = c
        ok |= b == ch
    m = n - k + 1
    cs = np.concatenate([[0], np.cumsum(ok)])
    valid = (cs[k:] - cs[:m]) == k
    if k <= 32:
        cc = code.astype(np.uint64)
        f, r = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
        two, sh = np.uint64(2), lambda j: np.uint64(2 * j)
    else:
        cc = code.astype(object)
        f, r = np.zeros(m, dtype=object), np.zeros(m, dtype=object)
        two, sh = 2, lambda j: 2 * j
    for j in range(k):
        f = (f << two) | cc[j:j + m]
        r = r | ((cc[j:j + m] ^ two) << sh(j))
    pos = np.nonzero(valid)[0]
    return n, pos.tolist(), f[pos].tolist(), r[pos].tolist()


def revcomp_bases(a):
    comp = np.zeros(256, dtype=np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y
    return comp[a][::-1]


# ---------------------------------------------------------------------------
# world
# ---------------------------------------------------------------------------
class World:
    pass


def build_world(k, pairs, kept_set=None, seed=1, canonical=True, palindromes=0, uniform=None):
    """Contigs of sizes [rest] + SIZES through synth.decorate, `rest` grown until the distinct k-mers are at least as many as
    `pairs`; the pairs go to the k-mers through a seeded permutation, the k-mers beyond them get pairs of the same list again,
    cycled.  canonical=False: the tables hold forward-strand k-mers; those whose reverse complement also occurs are left out of
    both tables.  palindromes (even k): that many own-reverse-complement k-mers are planted; both counts of such a k-mer double
    at every position (uint32), so they take pairs whose double is in `kept_set` as well.
    uniform: a list of (length, pair or list of pairs alternating by position) -- every k-mer of contig i carries that pair
    (the saturation tiles); `pairs` is ignored then."""
    w = World()
    w.k, w.canonical = k, canonical
    if uniform is not None:
        return _uniform_world(w, k, uniform, seed)
    npairs = len(pairs)
    rest = max(2000, npairs - sum(max(0, n - k + 1) for n in SIZES) + 1200)
    while True:
        r = synth.rng(seed)
        raw = [synth.random_contig(r, n) for n in (rest,) + SIZES]
        for i in range(palindromes):
            h = synth.random_contig(r, k // 2)
            at = 700 + 97 * i
            raw[0][at:at + k] = np.concatenate([h, revcomp_bases(h)])
        w.contigs = synth.as_bytes(synth.decorate(r, raw))
        w.kmers = [contig_kmers(c, k) for c in w.contigs]
        fw = set()
        for _, _, f, _ in w.kmers:
            fw.update(f)
        if canonical:
            keys = set()
            for _, _, f, rr in w.kmers:
                keys.update(min(a, b) for a, b in zip(f, rr))
        else:
            rc = {}
            for _, _, f, rr in w.kmers:
                rc.update(zip(f, rr))
            keys = {x for x in fw if rc[x] not in fw}
        pal = sorted(x for x in keys if canonical and k % 2 == 0 and _is_pal(x, k))
        plain = sorted(keys - set(pal))
        if len(plain) >= npairs:
            break
        rest += npairs - len(plain) + 500
    perm = np.random.default_rng(seed + 77).permutation(len(plain)).tolist()
    w.pair_of = {plain[j]: pairs[i % npairs] for i, j in enumerate(perm)}
    if pal:
        dbl = [p for p in pairs if ((2 * p[0]) % U32, (2 * p[1]) % U32) in kept_set and p[0] and p[1]]
        for i, x in enumerate(pal):
            w.pair_of[x] = dbl[(i * 7919) % len(dbl)]
    w.n_pal = len(pal)
    _tables(w)
    return w


def _is_pal(x, k):
    r = 0
    y = x
    for _ in range(k):
        r = (r << 2) | ((y & 3) ^ 2)
        y >>= 2
    return r == x


def _tables(w):
    keys = sorted(w.pair_of)
    w.R = {x: w.pair_of[x][0] for x in keys if w.pair_of[x][0] > 0}
    w.A = {x: w.pair_of[x][1] for x in keys if w.pair_of[x][1] > 0}
    w.keys = keys


def _uniform_world(w, k, uniform, seed):
    """contig i: random bases, all its canonical k-mers distinct from every other contig's (checked), pair by position"""
    r = synth.rng(seed)
    w.contigs = [synth.random_contig(r, n).tobytes() for n, _ in uniform]
    w.kmers = [contig_kmers(c, k) for c in w.contigs]
    w.pair_of = {}
    for (_, pos, f, rr), (_, spec) in zip(w.kmers, uniform):
        spec = spec if isinstance(spec, list) else [spec]
        for p, a, b in zip(pos, f, rr):
            x = min(a, b)
            assert x not in w.pair_of and a != b, "a repeated k-mer in a uniform contig: choose another seed"
            w.pair_of[x] = spec[p % len(spec)]
    w.n_pal = 0
    _tables(w)
    return w


def tables(w):
    """(read kmers, read values), (asm kmers, asm values) as sorted numpy arrays (k <= 32), or lists of Python ints"""
    out = []
    for d in (w.R, w.A):
        ks = sorted(d)
        vs = np.array([d[x] for x in ks], dtype=np.uint32)
        out.append((np.array(ks, dtype=np.uint64) if w.k <= 32 else ks, vs))
    return out


# ---------------------------------------------------------------------------
# exact reference
# ---------------------------------------------------------------------------
class Ref:
    pass


def reference(w, cfg, per_position=False):
    """-hist of the world: value(fmer) + value(rmer) in uint32 arithmetic from the two dictionaries (a canonical table holds one
    strand of a k-mer, so that sum is its value -- twice for an own-reverse-complement k-mer), K* per distinct pair, bins in
    Counters, koverCpy as the exact rational S and as the integer F of kfix units, per contig and in total."""
    R, A = w.R, w.A
    ref = Ref()
    ref.undr, ref.over = Counter(), Counter()
    ref.contig_kasm, ref.contig_kmissing, ref.contig_S, ref.contig_F, ref.contig_n_under = [], [], [], [], []
    ref.seen = Counter()
    ref.pp = []
    memo = {}
    for n, pos, f, rr in w.kmers:
        kmis = 0
        mine = Counter()
        for a, b in zip(f, rr):
            mine[((R.get(a, 0) + R.get(b, 0)) % U32, (A.get(a, 0) + A.get(b, 0)) % U32)] += 1
        S, F, nu = Fraction(0), 0, 0
        for pair, cnt in mine.items():
            e = memo.get(pair)
            if e is None:
                e = memo[pair] = evaluate(pair[0], pair[1], cfg)
            kind = e[3]
            if kind == "m":
                kmis += cnt
            elif kind == "u":
                ref.undr[e[5]] += cnt
                S += cnt * Fraction(e[6])
                F += cnt * kfix(e[6])
                nu += cnt
            else:
                ref.over[e[5]] += cnt
        ref.seen.update(mine)
        ref.contig_kasm.append(len(pos))
        ref.contig_kmissing.append(kmis)
        ref.contig_S.append(S)
        ref.contig_F.append(F)
        ref.contig_n_under.append(nu)
        if per_position:
            valid = np.zeros(n, dtype=bool)
            rk, ak, km = np.zeros(n), np.zeros(n), np.zeros(n)
            for p, a, b in zip(pos, f, rr):
                e = memo[((R.get(a, 0) + R.get(b, 0)) % U32, (A.get(a, 0) + A.get(b, 0)) % U32)]
                valid[p] = True
                rk[p], ak[p], km[p] = e[0], e[1], kmetric(e[0], e[1])
            ref.pp.append((valid, rk, ak, km))
    ref.memo = memo
    ref.kasm, ref.kmissing = sum(ref.contig_kasm), sum(ref.contig_kmissing)
    ref.S, ref.F, ref.n_under = sum(ref.contig_S, Fraction(0)), sum(ref.contig_F), sum(ref.contig_n_under)
    return ref


def dense(counter, n=None):
    n = (max(counter) + 1 if counter else 0) if n is None else n
    a = np.zeros(n, dtype=np.uint64)
    for i, v in counter.items():
        a[i] = v
    return a


def trim(a):
    a = np.asarray(a)
    nz = np.nonzero(a)[0]
    return a[: (nz[-1] + 1 if len(nz) else 0)]
