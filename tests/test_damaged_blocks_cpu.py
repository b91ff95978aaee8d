"""tests/damaged_blocks.py without a device: the valid catalogue decodes to its own arrays and shows no class, every damaged file shows
exactly the class it is made for and differs from the file it is made from in the fields meant and in nothing else.

What the host takes before a block reaches the decoder of -merge / -join (csrc/mfx_db_windows.cpp: every call opens its inputs with
merge_open_input, which applies mfx_db.cpp's flat_header_problem and read_delta_directory):
  header   magic MFXKMER1, 1 <= k <= 31, the delta flag (4) set and the placed flag (8) clear -- a placed, packed or plain file is refused;
           the canonical flag (1) and the other bits are not looked at; n_escape <= n and both within the file's size
  blocks   ceil(n / 4096) of them; kbits 0 .. 2k and vbits 2 .. 22 per block; offsets 8-byte aligned, each block exactly as long as its
           widths and length say; first k-mers below 4^k and strictly ascending
  escapes  k-mers below 4^k and STRICTLY ascending.  (The table loader, load_flat_escapes, asks for the first only.  A sorted file whose escape
           list repeats or descends is loaded into a table and refused by -merge and -join; every writer lists the escapes in the file's
           order, and no file here is of that kind.)
Every file made by damaged_blocks -- the valid catalogue at kbits 0 .. 2k and vbits 2 .. 22 with the delta flag alone, and each damaged file,
whose header, directory and offsets are its source's -- lies inside these ranges: damaged_blocks.host_problem restates the checks and is
asserted for each of them, and the library's own header check (mfx_db_probe) takes each.

  name    what is changed                                                                        class
  zero    a count field made 0 (entries 0, 15, 16, 1023, 1024, 4095, the last of the last block)   zero
  dup     a difference field made 0 (the same entries but 0)                                       order
  reach   a block's last difference enlarged: the last k-mer = the next block's first, and + 1     order
  wide    last block: a difference that takes a k-mer to 4^k, and to 4^k + 1                       order
  wrap    k = 31, kbits 62: the running sum passes 2^64 and comes back                             order
  lost    an escape field's list entry removed, or its k-mer moved by 1                            escape
  stale   one more list entry that no field refers to                                              none
  two     zero in one file, dup in another                                                         zero | order"""
import numpy as np
import pytest

from tests import damaged_blocks as dm
from tests import delta_blocks as db

KS = (15, 21, 31)


def _m():
    import merfin_amd as m
    m.load_library()
    return m


@pytest.mark.parametrize("k", KS)
def test_valid_catalogue_decodes_and_shows_nothing(k, tmp_path):
    m = _m()
    cases, src = dm.valid_cases(k), db.synthetic(k)
    assert len(cases) == len(src) and [c.name for c in cases] == [c.name for c in src]
    assert any(0 in c.counts for c in src) and not any(0 in c.counts for c in cases)
    for c, s in zip(cases, src):
        assert c.kmers == s.kmers and c.blocks() == s.blocks(), c.name
        assert [v for v, w in zip(c.counts, s.counts) if w] == [w for w in s.counts if w], c.name
        path = c.write(str(tmp_path / (c.name + ".mfxk")))
        assert db.decode_delta(path) == (k, c.kmers, c.counts), c.name
        assert dm.classify(path) == set(), c.name
        assert dm.host_problem(path) is None, c.name
        assert m.db_probe(path) == {"k": k, "format": "flat", "n_kmers": len(c.kmers)}, c.name


def _entries(raw):
    """per record: a block's first k-mer, or the difference to the record before it"""
    return [x if i % db.BLOCK == 0 else x - raw.records[i - 1] for i, x in enumerate(raw.records)]


def _differs_as_meant(path, src, diffs, fields, escapes):
    got = db.decode_raw(path, matched=False)
    want_e, want_f = _entries(src.raw), list(src.raw.fields)
    for i, v in diffs.items():
        assert want_e[i] != v
        want_e[i] = v
    for i, v in fields.items():
        assert want_f[i] != v
        want_f[i] = v
    assert got.k == src.k and got.flags == src.raw.flags and got.widths == src.raw.widths
    assert _entries(got) == want_e
    assert got.fields == want_f
    assert got.escapes == (src.raw.escapes if escapes is None else escapes) and (escapes is None or escapes != src.raw.escapes)
    if escapes is None:
        assert len(open(path, "rb").read()) == len(src.data)


@pytest.mark.parametrize("k", KS)
def test_damaged_files_show_their_class_and_nothing_else(k, tmp_path):
    m = _m()
    all_ = dm.damages(k)
    names = [d.name for d in all_]
    assert len(set(names)) == len(names)
    for kind in ("plain", "esc") + (("wrap",) if k == 31 else ()):
        path = dm.base(k, kind).write(str(tmp_path / (kind + ".mfxk")))
        assert dm.classify(path) == set() and dm.host_problem(path) is None
        b = dm.base(k, kind)
        assert db.decode_delta(path) == (k, b.kmers, b.counts)
    assert [n for n in names if n.startswith("wrap")] == (["wrap"] if k == 31 else [])
    for d in all_:
        if d.name == "two":
            paths = d.write(tmp_path)
            for p, want, df, fl in zip(paths, d.expected, d.diffs, d.fields):
                assert dm.classify(p) == want and dm.host_problem(p) is None
                _differs_as_meant(p, d.source, df, fl, None)
            continue
        path = d.write(tmp_path)
        assert dm.classify(path) == d.expected, d.name
        assert dm.host_problem(path) is None, d.name
        assert m.db_probe(path) == {"k": k, "format": "flat", "n_kmers": len(d.source.kmers)}, d.name
        _differs_as_meant(path, d.source, d.diffs, d.fields, d.escapes)
        assert len(d.diffs) + len(d.fields) + (d.escapes is not None) >= 1


@pytest.mark.parametrize("k", KS)
def test_the_damages_stand_where_they_are_meant_to(k):
    """every place of the list is used by every damage that can stand there, in block 0 and in a later block; the base file has the widths
    and the escapes the damages rely on; partner(k) puts a window boundary between a block's first k-mer and its record OUTSIDE"""
    m = _m()
    by = {}
    for d in dm.damages(k):
        by.setdefault(d.name.split("-")[0], []).append((d.block, d.entry))
    entries = {0, 15, 16, 1023, 1024, 4095}
    assert {e for b, e in dm.PLACES if b == 0} == entries and {e for b, e in dm.PLACES if b > 0} == entries and (2, dm.LAST - 1) in dm.PLACES
    assert sorted(by["zero"]) == sorted(dm.PLACES) and sorted(by["dup"]) == sorted(p for p in dm.PLACES if p[1])
    assert sorted(set(by["lost"])) == sorted(dm.PLACES + (dm.OUTSIDE,)) and len(by["lost"]) == 2 * len(dm.PLACES) + 1
    assert sorted(by["reach"]) == [(0, 4095)] * 2 + [(1, 4095)] * 2 and len(by["wide"]) == 4 and by["stale"] and by["two"]
    plain, esc = dm.base(k, "plain"), dm.base(k, "esc")
    assert plain.kmers == esc.kmers and [len(plain.kmers)] == [2 * db.BLOCK + dm.LAST]
    assert plain.widths == [(9, 3), (min(33, 2 * k - 4), 12), (2 * k, 22)]
    for b in range(3):                                             # wider than the narrowest in blocks 0 and 2, the narrowest in block 1
        kmin = db.min_widths(plain.kmers[b * db.BLOCK:(b + 1) * db.BLOCK], [])[0]
        assert (kmin < plain.widths[b][0]) == (b != 1)
    assert min(y - x for x, y in zip(plain.kmers, plain.kmers[1:])) >= 2
    for b in range(3):                                             # dup and wide move every record behind them: no escape of the plain file is among them
        assert [e for e in range(plain.blocks[b][4]) if plain.raw.fields[b * db.BLOCK + e] is None] == list(dm.EARLY)
    keys, vals = dm.partner(k)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and vals.min() >= 1 and len(keys) > db.BLOCK
    shared = len(np.intersect1d(keys, np.array(plain.kmers, dtype=np.uint64)))
    assert 0.4 * len(plain.kmers) < shared < 0.6 * len(plain.kmers)
    b, e = dm.OUTSIDE
    assert plain.kmers[b * db.BLOCK] < int(keys[db.BLOCK]) < plain.kmers[b * db.BLOCK + e]
    firsts = [np.array(plain.kmers[::db.BLOCK], dtype=np.uint64), keys[::db.BLOCK]]
    plan = m.db_merge_plan(firsts, [len(plain.kmers), len(keys)], k, 1)
    lo, hi = next((w[0], w[1]) for w in plan if w[0] <= plain.kmers[b * db.BLOCK] < w[1])
    assert hi == int(keys[db.BLOCK]) and hi <= plain.kmers[b * db.BLOCK + e]
