"""Blocks no writer makes, for the decoder of -merge and -join (csrc/mfx_merge.hip: mfx_delta_decode_kernel), built on
tests/delta_blocks.py: the catalogue of valid blocks with every zero count made 1 (valid_cases), an independent validator of a file
in plain Python ints (classify), and a list of damages (damages), each applied to a valid three-block file by changing the bits of
single fields or the escape list behind the blocks.  Header, directory, widths and offsets of every file made here stay as the host
checks of the library take them (host_problem restates those checks); only what a block's payload and the escape list SAY changes.

The three classes are the decoder's (csrc/mfx_kernels.h MFX_MERGE_ERR_*):
  order   a difference of 0; a k-mer at or above the next block's first; in the last block a k-mer at or above 4^k
  escape  a count field of all ones whose k-mer is not in the escape list
  zero    a count field of 0
tests/test_damaged_blocks_cpu.py checks the tools here, tests/test_gpu_decode_blocks.py runs the files through the device."""
import collections
import os
import struct
import tempfile

import numpy as np

from tests import delta_blocks as db

BLOCK = db.BLOCK
TEXT = {"order": "k-mers that do not ascend below the next block's first", "escape": "an escaped count that is not in the escape list",
        "zero": "a count of zero"}                                # the words of mfx_db_windows.cpp for each class


# ---- the valid catalogue ----
def valid_cases(k):
    """every Case of delta_blocks.synthetic(k) with each count of 0 made 1 (the merge refuses a zero count); k-mers and widths as they are"""
    src = db.synthetic(k)
    out = [db.Case(c.name, c.k, c.kmers, [v or 1 for v in c.counts], c.widths) for c in src]
    assert len(out) == len(src) and all(a.blocks() == b.blocks() for a, b in zip(out, src))
    return out


# ---- what a file shows ----
def classify(path):
    """the set of {"order", "escape", "zero"} the file at path shows (empty: a valid file), in Python ints: no sum wraps"""
    r = db.decode_raw(path, matched=False)
    listed = {x for x, _ in r.escapes}
    n, end, found = len(r.records), 1 << (2 * r.k), set()
    for b in range(0, n, BLOCK):
        limit = r.records[b + BLOCK] if b + BLOCK < n else end
        for i in range(b, min(b + BLOCK, n)):
            x, f = r.records[i], r.fields[i]
            if (i > b and x <= r.records[i - 1]) or x >= limit:
                found.add("order")
            if f is None and x not in listed:
                found.add("escape")
            if f == 0:
                found.add("zero")
    return found


def host_problem(path):
    """what the host checks in front of the merge (mfx_db.cpp: flat_header_problem, read_delta_directory; mfx_db_windows.cpp: merge_open_input) refuse in the
    file, restated; None: they take it.  (db.decode_raw asserts the block count, the offsets and the file's length.)"""
    raw, k, flags, n, n_esc = db.read_flat(path)
    r = db.decode_raw(path, matched=False)
    if not 1 <= k <= 31 or not flags & db.F_DELTA or flags & db.F_PLACED:
        return "header"
    if n_esc > n or n == 0:
        return "counts"
    for b, (kb, vb) in enumerate(r.widths):
        if kb > 2 * k or not 2 <= vb <= db.MAX_VBITS:
            return "widths of block %d" % b
    firsts = r.records[::BLOCK]
    if any(y <= x for x, y in zip(firsts, firsts[1:])) or firsts[-1] >> (2 * k):
        return "directory"
    ek = [x for x, _ in r.escapes]
    if any(y <= x for x, y in zip(ek, ek[1:])) or any(x >> (2 * k) for x in ek):
        return "escape list"
    return None


# ---- the files the damages are applied to ----
LAST = 1025                                                        # records of the last block
PLACES = ((0, 0), (0, 15), (0, 16), (0, 1023), (0, 1024), (0, 4095), (1, 4095), (2, 0), (2, 15), (2, 16), (2, 1023), (2, LAST - 1))
OUTSIDE = (1, 3000)                                                # a record behind a block first k-mer of partner(k): see there
EARLY = (3, 7)                                                     # the entries whose counts escape in every block of the plain file


class Base:
    """a valid file: kmers, counts, widths [(kbits, vbits)], data (its bytes), blocks [(first, offset, kbits, vbits, length, words of
    differences)], end (where the escape list begins)"""

    def __init__(self, k, kmers, counts, widths):
        self.k, self.kmers, self.counts, self.widths = k, kmers, counts, widths
        fd, path = tempfile.mkstemp(suffix=".mfxk")
        os.close(fd)
        try:
            db.encode_counts(path, k, kmers, counts, widths)
            self.data = open(path, "rb").read()
            self.raw = db.decode_raw(path)
        finally:
            os.unlink(path)
        n = len(kmers)
        (nblocks,) = struct.unpack_from("<Q", self.data, 32)
        d = struct.unpack_from("<%dQ" % (2 * (nblocks + 1)), self.data, 40)
        self.blocks = []
        for b in range(nblocks):
            kb, vb, cnt = (d[2 * b + 1] >> 48) & 0xff, d[2 * b + 1] >> 56, min(BLOCK, n - b * BLOCK)
            self.blocks.append((d[2 * b], d[2 * b + 1] & db.M48, kb, vb, cnt, ((cnt - 1) * kb + 63) // 64))
        self.end = d[2 * nblocks + 1] & db.M48
        assert self.raw.records == kmers and self.raw.widths == widths

    def diff(self, i):
        return self.kmers[i] - self.kmers[i - 1]

    def write(self, path):
        with open(path, "wb") as f:
            f.write(self.data)
        return path


_bases = {}


def base(k, kind):
    """kind "plain": two full blocks and one of 1025 records at widths (9, 3), (min(33, 2k - 4), 12), (2k, 22) -- wider than the narrowest in
    the first and the last --, every difference 2 or more, the counts of PLACES in the fields and those of EARLY escaped;
    "esc": the same k-mers with the counts of PLACES and OUTSIDE escaped as well;
    "wrap" (k = 31): a full block and a last one of 33 records, first k-mer 2^61, written at 62 bits"""
    if (k, kind) in _bases:
        return _bases[(k, kind)]
    rng = np.random.default_rng(9000 + k)
    K2 = 2 * k
    if kind == "wrap":
        assert k == 31
        kmers = db._block(7, [1] * (BLOCK - 1)) + db._block(1 << 61, [3] * 32)
        counts = [1 + i % 2 for i in range(BLOCK)] + [1 + i % 30 for i in range(33)]
        widths = [(1, 2), (62, 5)]
    else:
        kb1 = min(33, K2 - 4)
        d1 = [int(x) for x in rng.integers(2, 64, BLOCK - 1)]
        d1[1999] = 1 << (kb1 - 1)                                  # (entry 2000: none of PLACES)
        b0 = db._block(1000, [int(x) for x in rng.integers(2, 32, BLOCK - 1)])
        b1 = db._block(b0[-1] + 40, d1)
        b2 = db._block(b1[-1] + 100, [int(x) for x in rng.integers(2, 1024, LAST - 1)])
        kmers, widths, counts = b0 + b1 + b2, [(9, 3), (kb1, 12), (K2, 22)], []
        assert kmers[-1] < (1 << K2) - 2
        for b, (_, vb) in enumerate(widths):
            esc = (1 << vb) - 1
            c = [int(x) for x in rng.integers(1, esc, BLOCK if b < 2 else LAST)]
            c[EARLY[0]], c[EARLY[1]] = esc, (1 << 32) - 1
            if kind == "esc":
                for pb, e in PLACES + (OUTSIDE,):
                    if pb == b:
                        c[e] = esc + e % 5 if e % 2 else (1 << 31) + e
            counts += c
    _bases[(k, kind)] = Base(k, kmers, counts, widths)
    return _bases[(k, kind)]


def partner(k):
    """(k-mers, counts) of a valid database for the library's writer that interleaves with base(k, ..): every second k-mer of it, and
    behind every fourth one a k-mer it does not hold.  Its second block's first k-mer lies inside the base's block 1, in front of
    entry OUTSIDE[1]: under MFX_MERGE_RANGE=1 that record is outside the window of its own block's first k-mer."""
    src = base(k, "plain").kmers
    keys = np.array(sorted(src[::2] + [x + 1 for x in src[1::4]]), dtype=np.uint64)
    vals = (1 + np.arange(len(keys)) % 9).astype(np.uint32)
    vals[5::501] = (1 << 22) + 5
    return keys, vals


# ---- the damages ----
Damage = collections.namedtuple("Damage", "name write expected block entry source diffs fields escapes")
# write(directory) -> the damaged file's path (two: the two paths); expected: the set of classes (two: one set per file);
# source: the Base it is made from; diffs / fields {record index: the field's new value} and escapes (the new list, or None): ALL that changes


def _poke(data, off, bit, nbits, x):
    assert 0 <= x < 1 << nbits
    at, sh = off + (bit >> 6) * 8, bit & 63
    nb = 16 if sh + nbits > 64 else 8
    w = int.from_bytes(data[at:at + nb], "little")
    data[at:at + nb] = ((w & ~(((1 << nbits) - 1) << sh)) | (x << sh)).to_bytes(nb, "little")


def apply(src, diffs=None, fields=None, escapes=None):
    """the bytes of src with the difference fields diffs and the count fields fields {record index: value} set, and the escape list
    replaced (n_escape with it); nothing else of the file moves"""
    data = bytearray(src.data)
    for i, x in (diffs or {}).items():
        first, off, kb, vb, cnt, nkw = src.blocks[i // BLOCK]
        assert i % BLOCK > 0 and i % BLOCK < cnt
        _poke(data, off, (i % BLOCK - 1) * kb, kb, x)
    for i, x in (fields or {}).items():
        first, off, kb, vb, cnt, nkw = src.blocks[i // BLOCK]
        assert i % BLOCK < cnt
        _poke(data, off + nkw * 8, (i % BLOCK) * vb, vb, x)
    if escapes is not None:
        del data[src.end:]
        data += np.array([x for x, _ in escapes], dtype="<u8").tobytes() + np.array([v for _, v in escapes], dtype="<u4").tobytes()
        data[24:32] = struct.pack("<Q", len(escapes))
    return bytes(data)


def _damage(name, expected, block, entry, src, diffs=None, fields=None, escapes=None):
    def write(directory):
        path = os.path.join(str(directory), "%s_k%d.mfxk" % (name, src.k))
        with open(path, "wb") as f:
            f.write(apply(src, diffs, fields, escapes))
        return path
    return Damage(name, write, expected, block, entry, src, diffs or {}, fields or {}, escapes)


def damages(k):
    """[Damage]: (name, path-writer, expected classes, block, entry, ...), see the module's text and the table in tests/test_damaged_blocks_cpu.py"""
    plain, esc = base(k, "plain"), base(k, "esc")
    out = []
    at = lambda b, e: b * BLOCK + e
    for b, e in PLACES:
        assert plain.raw.fields[at(b, e)] not in (None, 0)
        out.append(_damage("zero-b%de%d" % (b, e), {"zero"}, b, e, plain, fields={at(b, e): 0}))
    for b, e in PLACES:
        if e:
            out.append(_damage("dup-b%de%d" % (b, e), {"order"}, b, e, plain, diffs={at(b, e): 0}))
    for b in (0, 1):                                               # the block's last k-mer at the next block's first, and one above it
        i = at(b, BLOCK - 1)
        for extra, tag in ((0, "eq"), (1, "above")):
            out.append(_damage("reach-%s-b%d" % (tag, b), {"order"}, b, BLOCK - 1, plain, diffs={i: plain.kmers[i + 1] - plain.kmers[i - 1] + extra}))
    for e in (LAST - 1, 16):                                       # the last block: a k-mer of 4^k, and one above it (from entry 16: every one behind it too)
        i = at(2, e)
        for extra, tag in ((0, "eq"), (1, "above")):
            out.append(_damage("wide-%s-e%d" % (tag, e), {"order"}, 2, e, plain, diffs={i: (1 << (2 * k)) - plain.kmers[i - 1] + extra}))
    if k == 31:
        # differences of entries 13 .. 17 of the last block (across a lane's seam): four of 2^62 - 1 pass 2^64, the fifth brings the sum back
        # to what it was, mod 2^64: from entry 17 on the k-mers are the source's in 64-bit arithmetic, those of 13 .. 15 lie above 4^k
        w = base(k, "wrap")
        was = sum(w.diff(at(1, e)) for e in range(13, 18))
        d = {at(1, e): (1 << 62) - 1 for e in range(13, 17)}
        d[at(1, 17)] = (1 << 64) + was - 4 * ((1 << 62) - 1)
        out.append(_damage("wrap", {"order"}, 1, 13, w, diffs=d))
    for j, (b, e) in enumerate(PLACES + (OUTSIDE,)):
        i = at(b, e)
        x = esc.kmers[i]
        assert esc.raw.fields[i] is None
        what = "outside" if (b, e) == OUTSIDE else "b%de%d" % (b, e)
        out.append(_damage("lost-rm-" + what, {"escape"}, b, e, esc, escapes=[p for p in esc.raw.escapes if p[0] != x]))
        if (b, e) != OUTSIDE:
            step = 1 if j % 2 == 0 else -1                         # (every difference is 2 or more: x +- 1 is no record, the list still ascends)
            out.append(_damage("lost-mv-" + what, {"escape"}, b, e, esc, escapes=[(p[0] + step, p[1]) if p[0] == x else p for p in esc.raw.escapes]))
    x = plain.kmers[5000] + 1
    out.append(_damage("stale", set(), 1, 5000 - BLOCK, plain, escapes=sorted(plain.raw.escapes + [(x, 77)])))
    z, d = out[2], next(o for o in out if o.name == "dup-b0e16")    # zero-b0e16 | dup-b0e16
    assert z.name == "zero-b0e16"

    def write_two(directory):
        paths = [os.path.join(str(directory), "two%d_k%d.mfxk" % (i, k)) for i in (0, 1)]
        for p, o in zip(paths, (z, d)):
            with open(p, "wb") as f:
                f.write(apply(plain, o.diffs, o.fields, o.escapes))
        return paths
    out.append(Damage("two", write_two, [{"zero"}, {"order"}], 0, 16, plain, [z.diffs, d.diffs], [z.fields, d.fields], None))
    return out
