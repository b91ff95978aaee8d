"""The delta-coded flat database (mfx_db.cpp FLAT_DELTA / FLAT_PLACED) as a FILE FORMAT, independent of the library: a decoder, an
encoder and a re-encoder in plain Python ints, written from the format's description at the top of mfx_db.cpp, and a catalogue of
blocks at the widths, lengths and positions where the two kernels that decode them on the device (mfx_table_add_delta_kernel,
mfx_table_add_placed_kernel) split, join and carry: tests/test_delta_blocks_cpu.py checks the tools and the catalogue against the host
reader, tests/test_gpu_delta_blocks.py loads the catalogue into every kind of table.

The file: header {magic, k, flags, n, n_escape} (32 bytes), uint64 nblocks, the directory of nblocks + 1 entries {first stored number,
file offset (48 bits) | kbits << 48 | vbits << 56} (the last entry closes the last block), the blocks (8-byte aligned; count - 1
differences of kbits bits, then -- from the next word boundary -- count count fields of vbits bits, all LSB-first in little-endian
uint64 words; an all-ones count field is an escape), then the escaped k-mers (uint64) and their counts (uint32).  A block holds 4096
records, the last one what is left.  Any kbits from the widest difference of the block up to the record's width and any vbits in
2..22 that holds the block's fields below all ones is a valid file: the library's writer takes the smallest kbits and the vbits that
make block + escapes smallest."""
import struct

import numpy as np

BLOCK = 4096
MAX_VBITS = 22
F_CANONICAL, F_DELTA, F_PLACED = 1, 4, 8
M48 = (1 << 48) - 1


def read_flat(path):
    raw = open(path, "rb").read()
    magic, k, flags, n, n_esc = struct.unpack_from("<8sIIQQ", raw, 0)
    assert magic == b"MFXKMER1"
    return raw, k, flags, n, n_esc


def bits_at(words, bit, nbits):
    i, sh = bit >> 6, bit & 63
    x = int(words[i]) >> sh
    if sh + nbits > 64:
        x |= int(words[i + 1]) << (64 - sh)
    return x & ((1 << nbits) - 1)


# ---- the raw form: stored numbers and count FIELDS, nothing interpreted (a placed file's numbers are no k-mers, and the fields of
# ---- a placed 31-mer file hold count << 1 | strand bit) ----
class Raw:
    """k, flags, records (the stored numbers), fields (the count fields; None = escape), widths [(kbits, vbits)] per block,
    escapes [(k-mer, count)] in the file's order"""

    def __init__(self, k, flags, records, fields, widths, escapes):
        self.k, self.flags, self.records, self.fields, self.widths, self.escapes = k, flags, records, fields, widths, escapes


def decode_raw(path, matched=True):
    """matched=False: a file whose escape fields and escape list do not match (tests/damaged_blocks.py) is read as it is"""
    raw, k, flags, n, n_esc = read_flat(path)
    assert flags & F_DELTA
    (nblocks,) = struct.unpack_from("<Q", raw, 32)
    assert nblocks == (n + BLOCK - 1) // BLOCK
    d = [int(x) for x in np.frombuffer(raw, dtype="<u8", count=2 * (nblocks + 1), offset=40)]
    records, fields, widths = [], [], []
    for b in range(nblocks):
        first, info = d[2 * b], d[2 * b + 1]
        off, kb, vb = info & M48, (info >> 48) & 0xff, (info >> 56) & 0xff
        cnt = min(BLOCK, n - b * BLOCK)
        nkw, nvw = ((cnt - 1) * kb + 63) // 64, (cnt * vb + 63) // 64
        assert off % 8 == 0 and (d[2 * b + 3] & M48) - off == (nkw + nvw) * 8
        w = np.frombuffer(raw, dtype="<u8", count=nkw + nvw, offset=off).tolist()
        vw = w[nkw:]
        cur = first
        for e in range(cnt):
            if e and kb:
                cur += bits_at(w, (e - 1) * kb, kb)
            records.append(cur)
            v = bits_at(vw, e * vb, vb)
            fields.append(None if v == (1 << vb) - 1 else v)
        widths.append((kb, vb))
    end = d[2 * nblocks + 1] & M48
    assert len(raw) == end + 12 * n_esc
    ek = np.frombuffer(raw, dtype="<u8", count=n_esc, offset=end).tolist()
    ev = np.frombuffer(raw, dtype="<u4", count=n_esc, offset=end + 8 * n_esc).tolist()
    assert not matched or sum(f is None for f in fields) == n_esc
    return Raw(k, flags, records, fields, widths, list(zip(ek, ev)))


def decode_delta(path):
    """(k, stored numbers, counts): decode_raw with every escaped field resolved from the escape list (a k-mer-sorted file: the stored
    numbers are the k-mers)"""
    r = decode_raw(path)
    esc = dict(r.escapes)
    assert len(esc) == len(r.escapes)
    return r.k, r.records, [esc[x] if f is None else f for x, f in zip(r.records, r.fields)]


def put_bits(words, bit, nbits, x):
    assert 0 <= x < (1 << nbits)
    i, sh = bit >> 6, bit & 63
    words[i] |= (x << sh) & 0xffffffffffffffff
    if sh + nbits > 64:
        words[i + 1] |= x >> (64 - sh)


def min_widths(records, fields):
    """the narrowest (kbits, vbits) that hold a block: its widest difference, and its largest field below all ones"""
    kb = max([b - a for a, b in zip(records, records[1:])] + [0]).bit_length()
    top = max([f for f in fields if f is not None] + [0])
    return kb, max(2, (top + 1).bit_length())


def writer_vbits(values):
    """the vbits the library's writer takes for a block of these values: block + escapes smallest (a field costs vbits bits, an
    escape 12 bytes more; of two equal sizes the narrower field)"""
    best = None
    for vb in range(2, MAX_VBITS + 1):
        cost = len(values) * vb + 96 * sum(v >= (1 << vb) - 1 for v in values)
        if best is None or cost < best[0]:
            best = (cost, vb)
    return best[1]


def encode(path, k, records, fields, widths, escapes, flags):
    """records: the stored numbers, ascending (Python ints); fields: a count field or None (escape) per record; widths: None (the
    narrowest), a list of (kbits, vbits) per block, or a function (block, narrowest kbits, narrowest vbits) -> (kbits, vbits);
    escapes: [(k-mer, count)]; flags: the header's, as they are"""
    n = len(records)
    assert len(fields) == n and flags & F_DELTA and sum(f is None for f in fields) == len(escapes)
    nblocks = (n + BLOCK - 1) // BLOCK
    at = 32 + 8 + 16 * (nblocks + 1)
    directory, blocks = [], []
    for b in range(nblocks):
        rec, fld = records[b * BLOCK:(b + 1) * BLOCK], fields[b * BLOCK:(b + 1) * BLOCK]
        kmin, vmin = min_widths(rec, fld)
        kb, vb = (kmin, vmin) if widths is None else widths(b, kmin, vmin) if callable(widths) else widths[b]
        assert kmin <= kb <= 64 and vmin <= vb <= MAX_VBITS, (b, kmin, kb, vmin, vb)
        cnt = len(rec)
        nkw, nvw = ((cnt - 1) * kb + 63) // 64, (cnt * vb + 63) // 64
        w = [0] * (nkw + nvw + 1)
        if kb:
            for e in range(1, cnt):
                put_bits(w, (e - 1) * kb, kb, rec[e] - rec[e - 1])
        assert w[nkw] == 0
        esc = (1 << vb) - 1
        for e, f in enumerate(fld):
            assert f is None or 0 <= f < esc
            put_bits(w, nkw * 64 + e * vb, vb, esc if f is None else f)
        assert w[-1] == 0
        directory += [rec[0], at | (kb << 48) | (vb << 56)]
        blocks.append(np.array(w[:-1], dtype="<u8").tobytes())
        at += (nkw + nvw) * 8
    directory += [0, at]
    with open(path, "wb") as f:
        f.write(struct.pack("<8sIIQQ", b"MFXKMER1", k, flags, n, len(escapes)))
        f.write(struct.pack("<Q", nblocks))
        f.write(np.array(directory, dtype="<u8").tobytes())
        for blk in blocks:
            f.write(blk)
        f.write(np.array([e[0] for e in escapes], dtype="<u8").tobytes())
        f.write(np.array([e[1] for e in escapes], dtype="<u4").tobytes())


def reencode(src, dst, widths_for_block):
    """a library-written file, placed or not, written again with other widths: the same stored numbers, count fields, escapes and
    header.  widths_for_block(block, narrowest kbits, narrowest vbits) -> (kbits, vbits)"""
    r = decode_raw(src)
    encode(dst, r.k, r.records, r.fields, widths_for_block, r.escapes, r.flags)
    return r


def plan_widths(kmers, counts, widths):
    """(kbits, vbits) per block of a k-mer-sorted file: the narrowest kbits and the writer's vbits, or what widths (a list, or a
    function of them) says"""
    out = []
    for b in range((len(kmers) + BLOCK - 1) // BLOCK):
        rec, cnt = kmers[b * BLOCK:(b + 1) * BLOCK], counts[b * BLOCK:(b + 1) * BLOCK]
        kmin, vw = min_widths(rec, [])[0], writer_vbits(cnt)
        out.append((kmin, vw) if widths is None else widths(b, kmin, vw) if callable(widths) else widths[b])
    return out


def encode_counts(path, k, kmers, counts, widths=None, flags=F_DELTA):
    """a k-mer-sorted file of (k-mer, count): a count that does not fit its block's field below all ones escapes.  widths as for
    encode (a function gets the narrowest kbits and the WRITER's vbits); the fields follow from the vbits taken"""
    per_block = plan_widths(kmers, counts, widths)
    fields, escapes = [], []
    for i, (x, c) in enumerate(zip(kmers, counts)):
        vb = per_block[i // BLOCK][1]
        if c >= (1 << vb) - 1:
            fields.append(None)
            escapes.append((x, c))
        else:
            fields.append(c)
    encode(path, k, kmers, fields, per_block, escapes, flags)
    return per_block


# ---- what a table holds after a load ----
def expected(kmers, counts, claimed=None):
    """({k-mer: count}, dropped): count 0 is never stored; claimed (a set): the k-mers a sequence-only index holds -- any other is
    dropped and counted"""
    table, dropped = {}, 0
    for x, c in zip(kmers, counts):
        if c == 0:
            continue
        if claimed is not None and x not in claimed:
            dropped += 1
            continue
        table[x] = table.get(x, 0) + c
    return table, dropped


# ---- the catalogue for the FULL table: synthetic key sets (the full table takes any k-mer) ----
LENGTHS = (1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4096)
VBIT_CLASSES = (2, 3, 11, 12, 21, 22)
CARRY_ENTRIES = (5, 1023, 1024, 4095)        # lane 0; lane 63 of wave 0 (the last entry of the placed kernel's round 0); lane 0 of wave 1 (the first
#                                              entry of round 1); the last lane of wave 3 -- the difference of entry e is field e - 1


class Case:
    def __init__(self, name, k, kmers, counts, widths):
        self.name, self.k, self.kmers, self.counts, self.widths = name, k, kmers, counts, widths

    def write(self, path):
        self.written = encode_counts(path, self.k, self.kmers, self.counts, self.widths)
        return path

    def blocks(self):
        """(kbits, vbits, length) of every block as it is written, from the catalogue's own data"""
        w = plan_widths(self.kmers, self.counts, self.widths)
        return [(kb, vb, min(BLOCK, len(self.kmers) - b * BLOCK)) for b, (kb, vb) in enumerate(w)]


def _counts_for(vb, n, rng, every_escape=False):
    """counts of a block written at vbits vb: small ones, zeros, (1 << vb) - 2 (the largest that fits) and (1 << vb) - 1 (the smallest
    escape), and counts beyond 22 and 31 bits"""
    esc = (1 << vb) - 1
    if every_escape:
        return [esc + int(x) for x in rng.integers(0, 5, n)]
    c = [int(x) for x in rng.integers(0, esc, n)]
    for i, v in enumerate((esc - 1, esc, 0, esc - 1, esc + 1, (1 << 22) - 2, (1 << 22) - 1, 1 << 31, (1 << 32) - 1, 0, 1)):
        if 3 + 7 * i < n:
            c[3 + 7 * i] = v
    c[0] = esc - 1
    c[-1] = esc if n > 1 else esc - 1
    return c


def _block(start, diffs):
    out = [start]
    for d in diffs:
        out.append(out[-1] + d)
    return out


def synthetic(k):
    """the full-table catalogue at this k: [Case].  Every k-mer is below 4^k; blocks ascend."""
    rng = np.random.default_rng(4000 + k)
    K2 = 2 * k
    top = (1 << K2) - 1
    cases = []

    def ones(n):
        return [1] * n

    # ---- last-block lengths: a full block of 1-bit differences, then the last block at the widest kbits of {33, 2k - 1}
    for L in LENGTHS:
        kb = min(33, K2 - 1)
        first = _block(7, ones(BLOCK - 1))
        d = [int(x) for x in rng.integers(1, 1 << (kb - 13), L - 1)] if L > 1 else []
        if L > 2:
            d[L // 2 - 1] = (1 << kb) - 1 - (L % 3)               # the widest difference somewhere inside
        elif L == 2:
            d[0] = (1 << kb) - 1
        last = _block(first[-1] + 12345, d)
        assert last[-1] <= top
        vb = VBIT_CLASSES[LENGTHS.index(L) % len(VBIT_CLASSES)]
        counts = _counts_for(2, BLOCK, rng) + _counts_for(vb, L, rng)
        cases.append(Case("len%d" % L, k, first + last, counts, [(1, 2), (kb if L > 1 else 0, vb)]))
    cases.append(Case("n1", k, [top - 5], [9], None))                                   # one record as a whole database
    cases.append(Case("n1esc", k, [3], [(1 << 32) - 1], None))                          # ... and one escaped record
    # ---- 2k bits: first record 0, a later one 4^k - 1
    cases.append(Case("kbits2k", k, _block(0, ones(15)) + [top], _counts_for(3, 17, rng), [(K2, 3)]))
    # ---- field widths: one file, a block per class (the differences are small except the one that makes the width)
    recs, counts, widths = [], [], []
    at = 1000

    def add(kb_true, kb_written, vb, every_escape=False, n=BLOCK, vb_written=None):
        nonlocal at
        d = [int(x) for x in rng.integers(1, 1 << min(kb_true, 3), n - 1)] if kb_true > 1 else ones(n - 1)
        if kb_true > 1:
            d[int(rng.integers(0, n - 1))] = (1 << kb_true) - 1
            d[n - 2] = 1 << (kb_true - 1)
        blk = _block(at, d)
        at = blk[-1] + 3
        recs.extend(blk)
        counts.extend(_counts_for(vb, n, rng, every_escape))
        widths.append((kb_written, vb_written or vb))
    add(1, 1, 2)
    add(2, 2, 3)
    for kb, vb in ((31, 11), (32, 12), (33, 21)):
        add(min(kb, K2 - 4), min(kb, K2 - 4), vb)                 # (k = 15 has no such width: 26 bits there)
    add(1, K2, 22)                                                # a 1-bit block written at width 2k
    add(2, 2, 2, every_escape=True)                               # every count of the block escapes
    add(min(20, K2 - 4), min(20, K2 - 4) + 3, 3, vb_written=9)    # non-minimal kbits and vbits
    add(3, 3, 2, n=33)                                            # (the last block)
    assert at <= top
    cases.append(Case("widths", k, recs, counts, widths))
    # ---- prefix carry: differences of 1 except one large one, at the seams of the lanes, waves and rounds; sums crossing 2^32
    big = 1 << min(40, K2 - 4)
    recs, counts, widths = [], [], []
    at = 1
    for e in CARRY_ENTRIES:
        d = ones(BLOCK - 1)
        d[e - 1] = big + e
        blk = _block(at, d)
        at = blk[-1] + 1
        recs.extend(blk)
        counts.extend([1 + (i % 2) for i in range(BLOCK)])
        widths.append((big.bit_length(), 2))
    if K2 >= 36:                                                  # the running sum of the DIFFERENCES crosses 2^32 inside the block
        d = [int(x) for x in rng.integers(1 << 20, 1 << 21, BLOCK - 1)]
        blk = _block(at + 5, d)
        assert blk[-1] - blk[0] > (1 << 32) and blk[-1] <= top
        recs.extend(blk)
        counts.extend([1 + (i % 2) for i in range(BLOCK)])
        widths.append((21, 2))
    assert recs[-1] <= top
    cases.append(Case("carry", k, recs, counts, widths))
    # ---- ten blocks of alternating widths, first k-mers far apart (several blocks per workgroup under MFX_INGEST_GRID)
    recs, counts, widths = [], [], []
    for b in range(10):
        kb = 1 if b % 2 == 0 else K2 - 16
        d = ones(BLOCK - 1) if kb == 1 else [int(x) for x in rng.integers(1 << (kb - 1), 1 << kb, BLOCK - 1)]
        blk = _block(b * (top // 11) + 17 * b, d)
        assert blk[-1] < (b + 1) * (top // 11)
        recs.extend(blk)
        vb = 2 if b % 2 == 0 else 22
        counts.extend(_counts_for(vb, BLOCK, rng))
        widths.append((kb, vb))
    cases.append(Case("grid", k, recs, counts, widths))
    return cases


def launches_case(k):
    """a file of wide blocks (kbits min(42, 2k), vbits 22), 1.3 MB or more: several launches under the smallest staging lanes"""
    rng = np.random.default_rng(4100 + k)
    kb = min(42, 2 * k)
    per = ((BLOCK - 1) * kb + 63) // 64 * 8 + BLOCK * 22 // 8
    nb = -(-1300000 // per)
    recs, counts = [], []
    at = 11
    for b in range(nb):
        d = [int(x) for x in rng.integers(1, 1 << (2 * k - 20), BLOCK - 1)]
        blk = _block(at, d)
        at = blk[-1] + 1 + b
        recs.extend(blk)
        counts.extend(_counts_for(22, BLOCK, rng))
    assert recs[-1] < (1 << (2 * k))
    return Case("launches", k, recs, counts, [(kb, 22)] * nb), nb * per


def straddles(blocks):
    """of blocks [(kbits, vbits, length)]: does a difference field end exactly at a word boundary, does one cross it by one bit, and
    does a block's last difference field cross into its last word"""
    ends = cross1 = last = False
    for kb, _vb, n in blocks:
        if not kb:
            continue
        for i in range(n - 1):
            s = (i * kb) % 64 + kb
            ends |= s == 64
            cross1 |= s == 65
        if n > 1:
            last |= ((n - 2) * kb) % 64 + kb > 64
    return ends, cross1, last


# ---- the catalogue for the PLACED kernel: a library-written placed file's records, cut to the blocks that kernel splits ----
# (a stored number must be the placement number of a canonical k-mer, or the kernel refuses the record: the numbers come from the library's own
# converter, the choice of records, the blocks and the widths from here.)  The kernel takes a block in rounds of 1024 records, four per lane.
PLACED_CARRY_ENTRIES = (2, 255, 256, 1023, 1024, 4095)   # lane 0; the last lane of wave 0; the first of wave 1; the last entry of round 0; the first of
#                                                          round 1; the last lane of wave 3 in the last round


def placed_big(k):
    """the one large difference of a placed carry block: a 32nd of the stored numbers' range -- 2^40 at k = 21, more beyond"""
    return 1 << ((64 if k == 31 else max(2 * k + 3, 41)) - 5)


def twins(k, rng, n):
    """n pairs of canonical k-mers whose placement numbers differ in the strand bit alone: stored numbers 1 apart (k <= 30), or equal with the
    strand bits 0 and 1 in the count fields (k = 31) -- the recipe of tests/test_placed_db.py"""
    from tests.test_placed_db import model_encode, revcomp
    mm, out = k - 3, []
    while len(out) < n:
        j = int(rng.integers(0, 4))
        c = int(rng.integers(0, 1 << (2 * mm)))
        if revcomp(c, mm) == c:
            continue
        e = int(rng.integers(0, 64))
        left, right = e >> (2 * (3 - j)), e & ((1 << (2 * (3 - j))) - 1)
        a = (left << (2 * (mm + 3 - j))) | (c << (2 * (3 - j))) | right
        b = (left << (2 * (mm + 3 - j))) | (revcomp(c, mm) << (2 * (3 - j))) | right
        if a > revcomp(a, k) or b > revcomp(b, k):
            continue
        pa, pb = model_encode(k, a)[0], model_encode(k, b)[0]
        if pa >> 1 == pb >> 1 and pa != pb:
            out.append((a, b) if pa < pb else (b, a))
    return out


def window_neighbours(k, rng, n):
    """n pairs of canonical k-mers with the same window of k - 3 bases, the same three bases around it and the same strand, the window one base
    further right in the second: placement numbers 2 apart (stored numbers 2 apart at k <= 30, 1 apart at k = 31)"""
    from tests.test_placed_db import model_encode, revcomp
    mm, out = k - 3, []
    while len(out) < n:
        j = int(rng.integers(0, 3))
        c = int(rng.integers(0, 1 << (2 * mm)))
        e = int(rng.integers(0, 64))
        pair = []
        for jj in (j, j + 1):
            left, right = e >> (2 * (3 - jj)), e & ((1 << (2 * (3 - jj))) - 1)
            pair.append((left << (2 * (mm + 3 - jj))) | (c << (2 * (3 - jj))) | right)
        a, b = pair
        if a > revcomp(a, k) or b > revcomp(b, k):
            continue
        if model_encode(k, b)[0] - model_encode(k, a)[0] == 2:
            out.append((a, b))
    return out


def placed_cuts(k, records, kmers, big):
    """[(name, indices into the file's records, widths)]: the files of the placed kernel's catalogue.  records: the stored numbers of a
    library-written placed file (ascending; k = 31: a twin's number twice); kmers: the k-mers in the same order; big: the one large
    difference of a carry block (every other difference of the block is below big >> 4).  Needs a pair of twins, and (k <= 30) of
    window neighbours, at an index of 4096 or more."""
    n = len(records)
    rec_bits = 64 if k == 31 else max(2 * k + 3, 41)
    cuts = []
    for L in LENGTHS:                                              # every last-block length, behind a full block
        cuts.append(("len%d" % L, list(range(1000, 1000 + BLOCK + L)), None))
    cuts.append(("n1", [n // 2], None))
    # two-record last blocks of the narrowest fields: kbits 1 (twins; k = 31: 0, the twins' numbers are equal) and 2 (window neighbours; k = 31: 1)
    d = [y - x for x, y in zip(records, records[1:])]
    for gap, name in ((0, "twins"), (1, "neighbours")) if k == 31 else ((1, "twins"), (2, "neighbours")):
        i = next(i for i in range(BLOCK, n - 1) if d[i] == gap)
        cuts.append((name, list(range(i - BLOCK, i + 2)), None))
    # the carry: consecutive records, and one jump of big or more at the entry named
    idx, at = [], 0
    for e in PLACED_CARRY_ENTRIES:
        idx += list(range(at, at + e))
        t = at + e
        while records[t] - records[at + e - 1] < big:
            t += 1
        idx += list(range(t, t + BLOCK - e))
        at = t + BLOCK - e
    cuts.append(("carry", idx, None))
    # ten blocks of alternating widths (the narrowest | the record's own and 22), first records far apart
    idx = [i for b in range(10) for i in range(b * (n // 10), b * (n // 10) + BLOCK)]
    cuts.append(("grid", idx, lambda b, kb, vb: (kb, vb) if b % 2 == 0 else (rec_bits, MAX_VBITS)))
    return cuts


def write_cut(path, src, idx, widths):
    """the records idx of the library-written file src (a Raw), as a file of their own with src's header flags"""
    esc = dict(src.escapes)
    rec, fld = [src.records[i] for i in idx], [src.fields[i] for i in idx]
    escapes = [(src.kmers[i], esc[src.kmers[i]]) for i in idx if src.fields[i] is None]
    encode(path, src.k, rec, fld, widths, escapes, src.flags)
    return path


def placed_source(m, k, keys, counts, tmp):
    """keys (ascending) and counts as the library's placed file, decoded: a Raw with .kmers and .counts in the file's order.  k <= 30: the order
    of the placement numbers; k = 31 (65 bits, made inside the converter only): a placed file whose every count escapes lists its k-mers, in
    the file's order, as its escape list"""
    if k <= 30:
        order = keys[np.argsort(m.db_place_keys(k, keys), kind="stable")]
    else:
        m.db_write_flat(tmp + ".f", k, keys, np.full(len(keys), 1 << 31, dtype=np.uint32))
        assert m.db_convert_placed(tmp + ".f", tmp + ".p") == len(keys)
        order = np.array([e[0] for e in decode_raw(tmp + ".p").escapes], dtype=np.uint64)
        assert len(order) == len(keys)
    m.db_write_flat(tmp + ".flat", k, keys, counts)
    assert m.db_convert_placed(tmp + ".flat", tmp + ".placed") == len(keys)
    raw = decode_raw(tmp + ".placed")
    by_key = dict(zip(keys.tolist(), counts.tolist()))
    raw.kmers = order.tolist()
    raw.counts = [by_key[x] for x in raw.kmers]
    assert raw.flags & F_PLACED and len(raw.records) == len(raw.kmers)
    return raw
