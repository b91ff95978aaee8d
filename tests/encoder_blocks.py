"""A catalogue of sorted k-mer databases for the WRITERS of the delta-coded flat file (csrc/mfx_delta.h: the block rule; csrc/mfx_db.cpp:
the host writers; csrc/mfx_sort.hip: mfx_delta_plan_kernel and mfx_delta_pack_kernel, the device encoder of every FULL block), as
tests/delta_blocks.py is one for the decoders.  Every world is (k = 31, k-mers ascending, counts >= 1); every block of it is built so that
the writer must choose a NAMED (kbits, vbits, escapes), which the world records beside the arrays.  The expected bytes are those of
delta_blocks.encode_counts, the format in Python ints: tests/test_encoder_blocks_cpu.py shows that the names hold on that reference alone and
that both host writers give its bytes; tests/test_gpu_encoder_blocks.py sends the same catalogue through every device route.

Key widths.  kbits 1 .. 56 stand in two files of 56 full blocks, ascending and descending, with vbits cycling through 2 .. 22 at two
different offsets (other (kbits, vbits) pairs, other word offsets of the count part).  A block's differences are random up to
min(kbits, 40) bits, and up to four of them have exactly kbits bits: field 0, field 4094 (the last), the field that crosses a word boundary
with the fewest bits behind it and the one with the fewest in front of it (one bit where kbits is odd).  k = 31 bounds the sum of a file's
differences by 2^62, so kbits 57 .. 62 stand in small files of their own with as many full-width differences as that leaves: 8 of 57 and 4
of 58 bits, 2 of 59 and 1 of 60, 1 of 61, 1 of 62 (at least 2^61, on either kind of crossing; one file's last k-mer is 4^31 - 1), each
file twice with other vbits.

Count widths.  A block named vbits holds counts below 2^vbits - 1, half of them in the upper half of that range (so that no narrower field
is cheaper) and 2^vbits - 2 among them.  A field costs 4096 bits per bit of width, an escape 96: 42 counts that need one bit more stay
escapes, 43 widen the field; 128 that need three bits more and 256 that need six are exact ties, which the narrower width wins.  A block
whose every count is 2^22 - 1 or more takes vbits 2 and 4096 escapes.

Escape positions (the pack kernel compacts a block's escapes in 16 rounds of 256 lanes, four waves each): one at index 0, one at 4095, at
63 | 64 (two waves), at 255 | 256 | 257 (two rounds), 300 consecutive counts of 2^32 - 1 across a round's end, and blocks without an escape
between blocks with some.

Every file ends in a partial block, which the host closes from the carry the device hands back."""
import os
import tempfile

import numpy as np

from tests import delta_blocks as db

K = 31
BLOCK = db.BLOCK
TOP = (1 << (2 * K)) - 1
ALWAYS = ((1 << 22) - 1, 1 << 22, 1 << 31, (1 << 32) - 1)        # counts that escape at every width


class Block:
    """what a block was built for: kbits, vbits, the number of escapes, its length, the indices of its escapes, a label"""

    def __init__(self, kb, vb, nesc, n, esc_at, label):
        self.kb, self.vb, self.nesc, self.n, self.esc_at, self.label = kb, vb, nesc, n, esc_at, label


class World:
    def __init__(self, name):
        self.name, self.k, self.blocks = name, K, []
        self._keys, self._counts, self._at = [], [], 0

    def add(self, diffs, counts, kb, vb, esc_at, label="", gap=1):
        """a block of len(counts) k-mers, the first one `gap` above the last k-mer so far (the first of all: at gap - 1)"""
        assert len(diffs) == len(counts) - 1 and (not self.blocks or self.blocks[-1].n == BLOCK)
        keys = np.cumsum(np.array([self._at + gap - (0 if self.blocks else 1)] + list(diffs), dtype=object)).tolist()
        self._keys += keys
        self._counts += [int(c) for c in counts]
        self._at = keys[-1]
        self.blocks.append(Block(kb, vb, len(esc_at), len(counts), sorted(esc_at), label))
        assert self._at <= TOP, (self.name, kb)

    def done(self):
        assert self.blocks[-1].n < BLOCK                           # every file ends in a partial block
        self.kmers, self.counts = np.array(self._keys, dtype=np.uint64), np.array(self._counts, dtype=np.uint32)
        assert all(b > a for a, b in zip(self._keys, self._keys[1:])) and self.kmers.tolist() == self._keys
        assert (self.counts >= 1).all() and self.counts.tolist() == self._counts
        return self

    def full(self):
        return [b for b in self.blocks if b.n == BLOCK]


def crossing_field(kb, n=BLOCK):
    """a difference field, neither the first nor the last of n - 1, that crosses a word boundary with the fewest bits behind it (one where
    kbits is odd); None where kbits divides 64"""
    best = None
    for i in range(1, n - 2):
        s = (i * kb) % 64 + kb
        if s > 64 and (best is None or s < best[0]):
            best = (s, i)
    return best[1] if best else None


def late_crossing_field(kb, n=BLOCK):
    """... and the crossing field with the fewest bits in front of the boundary (one where kbits is odd): nearly all of it is shifted
    down into the next word"""
    best = None
    for i in range(1, n - 2):
        at = (i * kb) % 64
        if at + kb > 64 and (best is None or at > best[0]):
            best = (at, i)
    return best[1] if best else None


def diffs_for(kb, n, rng, wide=None):
    """n - 1 differences of at most kbits bits: random up to min(kbits, 40) bits; exactly kbits bits at `wide` (default: the first field, the
    last, and the two crossing ones above), all ones, the top bit alone, and both ends set"""
    if n < 2:
        return []
    d = [int(x) for x in rng.integers(1, 1 << min(kb, 40), size=n - 1)] if kb > 1 else [1] * (n - 1)
    if wide is None:
        wide = [0, n - 2] + ([crossing_field(kb, n), late_crossing_field(kb, n)] if n > 3 and crossing_field(kb, n) is not None else [])
    for j, i in enumerate(wide):
        d[i] = ((1 << kb) - 1, 1 << (kb - 1), (1 << (kb - 1)) | 1)[j % 3]
    assert max(d).bit_length() == kb and min(d) >= 1
    return d


def counts_for(vb, n, rng, escapes=None):
    """n counts of a block the writer codes at vbits vb: below 2^vb - 1, every second one of them in the upper half of that range, 2^vb - 2
    among them; escapes {index: count} are put in as they are"""
    top = (1 << vb) - 2
    lo = max(1, (1 << (vb - 1)) - 1)
    c = rng.integers(1, top + 1, size=n)
    c[::2] = rng.integers(lo, top + 1, size=len(c[::2]))
    c = [int(x) for x in c]
    free = [i for i in range(n) if not escapes or i not in escapes]
    c[free[len(free) // 2]] = top
    for i, v in (escapes or {}).items():
        c[i] = v
    return c


def some_escapes(vb, how_many, n, rng):
    """{index: count}: how_many escapes at random indices -- the smallest escape of this width (full blocks only: in a short block one such
    count can make a wider field cheaper), and counts that escape at every width"""
    at = sorted(int(i) for i in rng.choice(n, size=how_many, replace=False))
    vals = (((1 << vb) - 1,) if n == BLOCK else ()) + ALWAYS
    return {i: vals[j % len(vals)] for j, i in enumerate(at)}


def _plain_block(w, kb, vb, n, rng, nesc=0, label="", wide=None, gap=None):
    esc = some_escapes(vb, min(nesc, n), n, rng)
    w.add(diffs_for(kb, n, rng, wide), counts_for(vb, n, rng, esc), kb if n > 1 else 0, vb, list(esc), label, gap or 1 + int(rng.integers(0, 1000)))


def _key_width_files():
    out = []
    for name, kbs, off, tail in (("kb_up", range(1, 57), 0, 1000), ("kb_down", range(56, 0, -1), 10, 4095)):
        rng = np.random.default_rng(6200 + off)
        w = World(name)
        for j, kb in enumerate(kbs):
            _plain_block(w, kb, 2 + (kb - 1 + off) % 21, BLOCK, rng, nesc=j % 10, gap=1 if j == 0 else None)      # (both start at k-mer 0)
        _plain_block(w, 33, 7, tail, rng, nesc=3)
        out.append(w.done())
    # 57 .. 62 bits: the wide differences first, last and on crossings, then as many more as the bound leaves
    for variant, off in (("a", 0), ("b", 11)):
        rng = np.random.default_rng(6300 + off)
        for kbs, tail in (((57, 58), 2), ((59, 60), 63), ((61,), 1), ((62,), 257)):
            w = World("kb%s%s" % ("_".join(map(str, kbs)), variant))
            for kb in kbs:
                many = {57: 8, 58: 4, 59: 2, 60: 1, 61: 1, 62: 1}[kb]
                cross = crossing_field(kb)
                wide = ([0, BLOCK - 2, cross, late_crossing_field(kb)] + [int(i) for i in rng.choice(np.arange(5, 4000), size=8, replace=False)])[:many]
                if many == 1:
                    wide = [(late_crossing_field(kb) if variant == "a" else cross) if kb == 62 else (0 if variant == "a" else BLOCK - 2)]
                diffs = diffs_for(kb, BLOCK, rng, wide)
                if kb == 62:                                       # at least 2^61, and room below 4^31 for the rest of the file
                    diffs[wide[0]] = (1 << 61) | (1 << 30) | 1
                vb = 2 + (kb - 1 + off) % 21
                esc = some_escapes(vb, (kb + off) % 7, BLOCK, rng)
                w.add(diffs, counts_for(vb, BLOCK, rng, esc), kb, vb, list(esc), "wide%d" % many, 1)
            if kbs == (62,) and variant == "a":                    # the file's last k-mer is the largest 31-mer
                n = tail
                d = diffs_for(20, n, rng)
                gap = TOP - w._at - sum(d)
                assert gap >= 1
                w.add(d, counts_for(5, n, rng), 20, 5, [], "top", gap)
                assert w._at == TOP
            else:
                _plain_block(w, 9, 3 + off, tail, rng, nesc=min(1, tail - 1))
            out.append(w.done())
    return out


def _needing(bits, how_many, rng):
    """counts whose field needs exactly `bits` bits: bit_length(count + 1) == bits, both ends of that range among them"""
    lo, hi = (1 << (bits - 1)) - 1, (1 << bits) - 2
    v = [int(x) for x in rng.integers(lo, hi + 1, size=how_many)]
    v[0], v[-1] = lo, hi
    return v


def _count_width_file():
    rng = np.random.default_rng(6400)
    w = World("cost_edges")

    def block(vb_base, extra_bits, how_many, named_vb, named_nesc, label, kb=17):
        at = sorted(int(i) for i in rng.choice(BLOCK, size=how_many, replace=False))
        vals = _needing(vb_base + extra_bits, how_many, rng)
        planted = dict(zip(at, vals))
        c = counts_for(vb_base, BLOCK, rng, planted)
        w.add(diffs_for(kb, BLOCK, rng), c, kb, named_vb, at if named_nesc else [], label, 5)

    for vb in (3, 11, 21):
        block(vb, 1, 42, vb, 42, "stay42")                         # 42 x 96 = 4032 < 4096: escapes
        block(vb, 1, 43, vb + 1, 0, "widen43")                     # 43 x 96 = 4128 > 4096: one bit more for every field
    for vb in (4, 12, 19):
        block(vb, 3, 128, vb, 128, "tie128")                       # 128 x 96 = 3 x 4096
    for vb in (3, 9, 16):
        block(vb, 6, 256, vb, 256, "tie256")                       # 256 x 96 = 6 x 4096
    c = [ALWAYS[int(i)] for i in rng.integers(0, len(ALWAYS), size=BLOCK)]
    c[0], c[-1] = (1 << 22) - 1, (1 << 32) - 1
    w.add(diffs_for(23, BLOCK, rng), c, 23, 2, list(range(BLOCK)), "all_escape", 5)
    esc = {9: (1 << 22) - 1, 10: (1 << 32) - 1, 4000: (1 << 32) - 1}
    c = counts_for(22, BLOCK, rng, esc)
    c[8] = (1 << 22) - 2                                           # the largest count a field holds, beside the smallest escape and the 33-bit bin
    w.add(diffs_for(45, BLOCK, rng), c, 45, 22, list(esc), "vb22", 5)
    _plain_block(w, 12, 22, 100, rng, nesc=2)
    return w.done()


def _escape_position_file():
    rng = np.random.default_rng(6500)
    w = World("escape_positions")
    big = (1 << 32) - 1

    def block(vb, at, label, kb=29, vals=None):
        esc = {i: (vals or ((1 << vb) - 1, big))[j % 2] for j, i in enumerate(at)}
        w.add(diffs_for(kb, BLOCK, rng), counts_for(vb, BLOCK, rng, esc), kb, vb, list(at), label, 3)

    block(6, [], "none")
    block(6, [0], "first")
    block(13, [], "none")
    block(13, [4095], "last")
    block(2, [63, 64], "waves")
    block(9, [], "none")
    block(9, [255, 256, 257], "rounds")
    block(4, list(range(200, 500)), "run300", vals=(big, big))     # across the end of round 0
    block(4, [], "none")
    block(20, list(range(1900, 2200)), "run300", vals=(big, big))  # across the end of round 7
    block(3, [0, 63, 64, 255, 256, 1023, 1024, 4094, 4095], "seams")
    block(3, [], "none")
    _plain_block(w, 29, 3, 4095, rng, nesc=5)
    return w.done()


_worlds = None
_bytes = {}


def worlds():
    """the catalogue: [World], built once and left unchanged"""
    global _worlds
    if _worlds is None:
        _worlds = _key_width_files() + [_count_width_file(), _escape_position_file()]
        assert len({w.name for w in _worlds}) == len(_worlds)
    return _worlds


def names():
    return [w.name for w in worlds()]


def world(name):
    return next(w for w in worlds() if w.name == name)


def expected_bytes(w):
    """the file the Python encoder (delta_blocks.encode_counts, narrowest kbits, the writer's vbits) makes of a world; made once"""
    if w.name not in _bytes:
        fd, path = tempfile.mkstemp(suffix=".mfxk")
        os.close(fd)
        try:
            w.written = db.encode_counts(path, w.k, w.kmers.tolist(), w.counts.tolist())
            with open(path, "rb") as f:
                _bytes[w.name] = f.read()
        finally:
            os.remove(path)
    return _bytes[w.name]
