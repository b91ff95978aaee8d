"""One deterministic world per k for the -hist worklist (tests/test_gpu_worklist.py; its CPU assertions: tests/test_worklist_world_cpu.py).

The recipe of tests/test_gpu_second_bucket.world -- < 300 kb in three contigs, none a multiple of the tile, a diverged satellite array
(home lines full of other k-mers), an exact tandem array, N runs, lower case; built at MFX_LOAD_FACTOR=0.5 -- with HOST-built tables (the
read database as made here, the assembly's k-mers counted by the oracle) and, on top of it, what the worklist's rare classes need:
  * the diverged array has 300 copies, not 120: with 120 no minimizer of the assembly has more than 31 k-mers, i.e. two lines of 16
    slots hold them all wherever the table is nearly empty (k = 31: 2^25 lines at least) and no query is displaced past the two
    cooperative passes; with 300 some twenty minimizers have 33 ... 43 (csrc/mfx_place.h on the host; tests/test_worklist_world_cpu.py);
  * saturated read counts: ~3000 distinct assembly k-mers, taken at random positions of all contigs (so of all four waves of a tile),
    get a read count from SAT_VALUES = {2047, 2048, 2500, 65535, 2^32 - 1}: their slot's 11-bit field is saturated, the count lives in
    the side table, and where the entry is not in the first two slots of its side line the position is LISTED (mode 2);
  * even k: 48 planted h + revcomp(h) palindromes over all contigs, six of them inside the diverged array, all with saturated read
    counts (a listed palindrome is the only way to the list's `dbl` bit);
  * a read filter max = READ_MAX = 3000 through the index's -min / -max route (applied at lookup): the saturated k-mers above it
    (65535, 2^32 - 1, and the exact tandem array's ~3500) are missing AND listed -- the rest kernel's tile -> contig arithmetic;
  * the last contig ends in a tile of 300 bases whose k-mers are all saturated: a wave with fewer than 64 wanted positions.
Everything else here is host arithmetic for the tests: the canonical k-mer of every position (numpy, checked against the oracle in the
CPU test), the tile of a position, the positions of a (tile, wave)."""
import numpy as np

from oracle import pyoracle as po
from tests import synth
from tests.test_kstar_grid_cpu import PC

PEAK = 17.3
FAR_PEAK = 5.0                                   # a second evaluation of the same tables: read counts of 2047 ... 3000 then fall into K* bins >= 1024 (far bins at nbins = 1024)
READ_MAX = 3000
SIZES = (150001, 98000, 4 * PC["tile"] + 300)    # 264 685 bases; the last contig ends in a tile of 300 bases
SAT_VALUES = (2047, 2048, 2500, 65535, 2 ** 32 - 1)
N_SAT = 3000
N_PAL = 48
KS = (19, 20, 21, 22, 26, 31)
TILE, BLOCK, FIELD = PC["tile"], PC["block"], PC["field"]
WAVES = BLOCK // 64
ARRAY_AT, ARRAY_UNIT, ARRAY_COPIES = 30000, 171, 300       # 51 300 bases of contig 1

_worlds = {}


def revcomp_bytes(b):
    return bytes(b.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1])


def canonical_positions(k, contig):
    """(kmer[n], ok[n], pal[n]) of a contig of n bytes: the canonical k-mer STARTING at every position (A=0 C=1 T=2 G=3, either case), whether
    all its k bases are ACGT, and whether it is its own reverse complement.  Entries with ok false are 0."""
    c = np.frombuffer(contig, dtype=np.uint8)
    n = len(c)
    code = ((c >> 1) & 3).astype(np.uint64)
    up = c & 0xDF
    valid = (up == ord("A")) | (up == ord("C")) | (up == ord("G")) | (up == ord("T"))
    m = max(n - k + 1, 0)
    f = np.zeros(m, dtype=np.uint64)
    r = np.zeros(m, dtype=np.uint64)
    for i in range(k):
        f |= code[i:i + m] << np.uint64(2 * (k - 1 - i))
        r |= (code[i:i + m] ^ np.uint64(2)) << np.uint64(2 * i)
    cs = np.concatenate([[0], np.cumsum(valid)])
    ok_m = (cs[k:k + m] - cs[:m]) == k
    kmer, ok, pal = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    kmer[:m] = np.where(ok_m, np.minimum(f, r), 0)
    ok[:m] = ok_m
    pal[:m] = ok_m & (f == r)
    return kmer, ok, pal


class World:
    """contigs (bytes), read = (kmers, counts) unfiltered, asm = (kmers, counts) from the oracle's counter; per contig the arrays of
    canonical_positions; sat: the sorted k-mers whose slot has a saturated field (read or assembly count >= 2047)"""

    def __init__(self, k):
        self.k = k
        r = synth.rng(9300 + k)
        truth = synth.make_truth(r, SIZES, tandem=(37, 200))        # an exact tandem array per long contig: read counts of ~3500
        arr = np.tile(synth.random_contig(r, ARRAY_UNIT), ARRAY_COPIES)
        mut = r.random(len(arr)) < 0.04
        arr[mut] = synth.BASES[r.integers(0, 4, size=int(mut.sum()))]
        truth[1][ARRAY_AT:ARRAY_AT + len(arr)] = arr
        asm = synth.decorate(r, synth.mutate(r, truth))
        asm[2][4 * TILE:] = truth[2][4 * TILE:]                      # the short last tile keeps all its k-mers (no N, no substitution)
        # even k: the palindromes go into the ASSEMBLY (after the substitutions, the N runs and the lower case), 61 apart from a multiple of
        # 997 so that they fall into all four waves; 24 / 14 / 4 over the contigs' tiles and 6 inside the diverged array
        self.pal_at = []
        if k % 2 == 0:
            spots = [(0, 5000 + 5981 * i + 61 * (i % 4)) for i in range(24)] + [(1, 83000 + 1001 * i + 61 * (i % 4)) for i in range(14)] + \
                    [(2, 700 + 4096 * i + 64 * i) for i in range(4)] + [(1, ARRAY_AT + 1000 + 8111 * i + 67 * (i % 4)) for i in range(6)]
            assert len(spots) == N_PAL
            for ci, at in spots:
                h = synth.random_contig(r, k // 2).tobytes()
                asm[ci][at:at + k] = np.frombuffer(h + revcomp_bytes(h), dtype=np.uint8)
                self.pal_at.append((ci, at))
        truth_b, self.contigs = synth.as_bytes(truth), synth.as_bytes(asm)
        rk, rv = synth.read_counts(r, k, truth_b, PEAK, err_kmers=2000)
        self.asm = po.count_kmers(k, self.contigs)
        self.pos = [canonical_positions(k, c) for c in self.contigs]
        # the saturated read counts: the k-mers of N_SAT random positions, of the planted palindromes and of the whole last tile of the last contig
        picks = []
        for ci, (km, ok, pal) in enumerate(self.pos):
            idx = np.nonzero(ok)[0]
            # (a quarter more positions than k-mers wanted: positions of the arrays share their k-mers)
            picks.append(km[r.choice(idx, size=5 * N_SAT * len(self.contigs[ci]) // (4 * sum(SIZES)) + 1, replace=False)])
        picks.append(np.array([self.pos[ci][0][at] for ci, at in self.pal_at], dtype=np.uint64))
        last = self.pos[2]
        tail = np.arange(4 * TILE, len(self.contigs[2]))
        picks.append(last[0][tail][last[1][tail]])
        sat_k = np.unique(np.concatenate(picks))
        sat_v = np.array([SAT_VALUES[i % len(SAT_VALUES)] for i in r.permutation(len(sat_k))], dtype=np.uint32)
        keep = ~np.isin(rk, sat_k)
        rk, rv = np.concatenate([rk[keep], sat_k]), np.concatenate([rv[keep], sat_v])
        o = np.argsort(rk)
        self.read = (rk[o], rv[o])
        self.planted = sat_k
        # read count of every assembly k-mer (0: absent), then the k-mers with a saturated field
        at = np.searchsorted(self.read[0], self.asm[0])
        at[at == len(self.read[0])] = 0
        self.asm_read = np.where(self.read[0][at] == self.asm[0], self.read[1][at], 0).astype(np.uint32)
        self.sat = self.asm[0][(self.asm_read >= FIELD) | (self.asm[1] >= FIELD)]
        self.sat_missing = self.asm[0][(self.asm_read >= FIELD) & (self.asm_read > READ_MAX)]
        self.tile0 = np.concatenate([[0], np.cumsum([(len(c) + TILE - 1) // TILE for c in self.contigs])])   # first tile of every contig
        self.ntiles = int(self.tile0[-1])
        self._slots = None

    # ---- positions ----
    def positions_in(self, ci, kmers):
        """the positions of contig ci whose canonical k-mer is one of the sorted `kmers`"""
        km, ok, _ = self.pos[ci]
        return np.nonzero(ok & np.isin(km, kmers))[0]

    def tile_of(self, ci, p):
        return self.tile0[ci] + np.asarray(p) // TILE

    def wave_of(self, p):
        return (np.asarray(p) % BLOCK) // 64

    def slot_kmers(self):
        """{(tile, wave): sorted array of the canonical k-mers of its positions, with repeats} -- the positions of wave w of a tile are
        b * 256 + 64 * w + lane, b = 0 ... 15, lane = 0 ... 63, from the tile's first position on"""
        if self._slots is not None:
            return self._slots
        out = {}
        for ci, (km, ok, _) in enumerate(self.pos):
            p = np.nonzero(ok)[0]
            key = self.tile_of(ci, p) * WAVES + self.wave_of(p)
            o = np.argsort(key, kind="stable")
            key, vals = key[o], km[p][o]
            cut = np.nonzero(np.diff(key))[0] + 1
            for s, e in zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(key)]])):
                out[(int(key[s]) // WAVES, int(key[s]) % WAVES)] = np.sort(vals[s:e])
        self._slots = out
        return out

    def tile_contig(self, tile):
        return int(np.searchsorted(self.tile0, tile, side="right") - 1)


def world(k):
    """shared by every test of a session; unchanged"""
    if k not in _worlds:
        _worlds[k] = World(k)
    return _worlds[k]
