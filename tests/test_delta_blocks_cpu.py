"""tests/delta_blocks.py against the library's host side (no device): what the Python encoder writes, the host reader behind
mfx_db_convert reads back; what the library writes, decoded and encoded again at the writer's widths, is the same file byte for
byte; the catalogue holds every class of block it names; and a placed 31-mer file whose neighbouring records lie 2^63 or more apart
-- a 64-bit difference field -- converts back to its k-mers and counts."""
import numpy as np
import pytest

from tests import delta_blocks as db
from tests.test_placed_db import canon


def _m():
    import merfin_amd as m
    m.load_library()
    return m


@pytest.fixture(scope="module")
def catalogues():
    return {k: db.synthetic(k) for k in (15, 21, 31)}


@pytest.mark.parametrize("k", [15, 21, 31])
def test_encoded_files_are_read_by_the_host_reader(k, catalogues, tmp_path):
    """every case of the full-table catalogue, written by the Python encoder at the catalogue's widths, through mfx_db_convert: the
    k-mers and counts it was made of (the converter writes the sorted form again, which the independent decoder reads)"""
    m = _m()
    for c in catalogues[k] + [db.launches_case(k)[0]]:
        src, out = str(tmp_path / (c.name + ".mfxk")), str(tmp_path / (c.name + ".out"))
        c.write(src)
        assert m.db_probe(src) == {"k": k, "format": "flat", "n_kmers": len(c.kmers)}, c.name
        assert m.db_convert(src, out) == len(c.kmers), c.name
        kk, keys, vals = db.decode_delta(out)
        assert kk == k and keys == c.kmers and vals == c.counts, c.name
        raw = db.decode_raw(src)                                # ... and the raw decoder reads the encoder's file as written
        assert raw.records == c.kmers and raw.widths == c.written, c.name
        assert raw.fields == [None if v >= (1 << c.written[i // db.BLOCK][1]) - 1 else v for i, v in enumerate(c.counts)], c.name


def _world(k, n, seed):
    r = np.random.default_rng(seed)
    km = canon(r, k, n)
    vals = (1 + (km % np.uint64(300))).astype(np.uint32)
    vals[::7] = 0
    vals[1::53] = (1 << 20) - 1
    vals[2::59] = (1 << 21) - 1
    vals[3::61] = 1 << 21
    vals[4::67] = (1 << 22) - 2
    vals[5::71] = (1 << 22) - 1
    vals[6::97] = 3000000011
    vals[4096:8192] = (vals[4096:8192] % 3).astype(np.uint32)   # a block of 2-bit fields in the sorted form
    return km, vals


@pytest.mark.parametrize("k,placed", [(21, False), (31, False), (4, False), (21, True), (30, True), (31, True)])
def test_library_files_encode_again_byte_for_byte(k, placed, tmp_path):
    """decode_raw of a library-written file, sorted or placed, then encode at the widths the writer takes: the same bytes"""
    m = _m()
    if k == 4:
        km = np.arange(3, 250, dtype=np.uint64)
        vals = (km % np.uint64(9)).astype(np.uint32)
    else:
        km, vals = _world(k, 9000, 600 + k)
    flat, lib, mine = (str(tmp_path / x) for x in ("flat.mfxk", "lib.mfxk", "mine.mfxk"))
    m.db_write_flat(flat, k, km, vals)
    if placed:
        assert m.db_convert_placed(flat, lib) == len(km)
    else:
        lib = flat
    raw = db.decode_raw(lib)
    assert bool(raw.flags & db.F_PLACED) == placed
    # the values the writer planned with: a field as it is; an escaped count as the escape list says (k = 31 placed: folded with the strand bit,
    # which cannot move a count of this world across a field's limit)
    esc = iter(raw.escapes)
    fold = placed and k == 31
    values = []
    for f in raw.fields:
        if f is None:
            c = next(esc)[1]
            f = c if not fold else 0xffffffff if c >= 1 << 21 else c << 1
        values.append(f)
    widths = []
    for b in range(len(raw.widths)):
        rec = raw.records[b * db.BLOCK:(b + 1) * db.BLOCK]
        widths.append((db.min_widths(rec, [])[0], db.writer_vbits(values[b * db.BLOCK:(b + 1) * db.BLOCK])))
    assert widths == raw.widths
    db.encode(mine, raw.k, raw.records, raw.fields, widths, raw.escapes, raw.flags)
    assert open(mine, "rb").read() == open(lib, "rb").read()
    # ... and written at other widths the host reader gives the same arrays
    wide, back = str(tmp_path / "wide.mfxk"), str(tmp_path / "back.mfxk")
    rec_bits = 64 if fold else (max(2 * k + 3, 41) if placed else 2 * k)
    db.reencode(lib, wide, lambda b, kb, vb: [(rec_bits, 22), (min(kb + 1, rec_bits), min(vb + 1, 22)), (kb, 22), (rec_bits, vb)][b % 4])
    assert m.db_convert(wide, back) == len(km)
    kk, keys, cnts = db.decode_delta(back)
    assert kk == k and keys == km.tolist() and cnts == vals.tolist()


def test_the_catalogue_holds_every_class_it_names(catalogues):
    for k, cases in catalogues.items():
        K2 = 2 * k
        blocks = [b for c in cases for b in c.blocks()]
        kbits, vbits = {b[0] for b in blocks}, {b[1] for b in blocks}
        assert {0, 1, 2, K2} <= kbits
        assert {31, 32, 33} & set(range(K2)) <= kbits
        assert set(db.VBIT_CLASSES) <= vbits and 9 in vbits
        for L in db.LENGTHS:                                      # every last-block length, behind a full block
            c = next(x for x in cases if x.name == "len%d" % L)
            assert [b[2] for b in c.blocks()] == [db.BLOCK, L]
        assert [len(c.kmers) for c in cases if c.name.startswith("n1")] == [1, 1]
        assert db.straddles(blocks) == (True, True, True)
        # a 1-bit block written at width 2k, and widths above the narrowest in both fields
        w = next(x for x in cases if x.name == "widths")
        assert any(kb == K2 and db.min_widths(w.kmers[b * db.BLOCK:(b + 1) * db.BLOCK], [])[0] == 1 for b, (kb, vb, n) in enumerate(w.blocks()))
        assert any(kb > db.min_widths(w.kmers[b * db.BLOCK:(b + 1) * db.BLOCK], [])[0] and vb == 9 for b, (kb, vb, n) in enumerate(w.blocks()))
        # both sides of every escape boundary: (1 << vbits) - 2 in the field, (1 << vbits) - 1 and 2^32 - 1 escaped; zero counts; a block of escapes only
        for vb in db.VBIT_CLASSES:
            seen = set()
            for c in cases:
                for b, (kb_, vb_, n) in enumerate(c.blocks()):
                    if vb_ == vb:
                        seen |= set(c.counts[b * db.BLOCK:b * db.BLOCK + n])
            assert {0, (1 << vb) - 2, (1 << vb) - 1} <= seen, (k, vb)
        assert any(all(v >= (1 << vb) - 1 for v in w.counts[b * db.BLOCK:b * db.BLOCK + n]) for b, (kb, vb, n) in enumerate(w.blocks()))
        assert (1 << 32) - 1 in w.counts and 1 << 31 in w.counts
        # the carry: one large difference per block, at each seam; a block whose differences sum beyond 2^32
        cy = next(x for x in cases if x.name == "carry")
        big = 1 << min(40, K2 - 4)
        assert k < 22 or big == 1 << 40
        for b, e in enumerate(db.CARRY_ENTRIES):
            rec = cy.kmers[b * db.BLOCK:(b + 1) * db.BLOCK]
            d = [y - x for x, y in zip(rec, rec[1:])]
            assert d[e - 1] >= big and sorted(d)[-2] == 1
        if K2 >= 36:
            rec = cy.kmers[4 * db.BLOCK:5 * db.BLOCK]
            assert rec[-1] - rec[0] > 1 << 32 and rec[1] - rec[0] < 1 << 32
        g = next(x for x in cases if x.name == "grid")
        assert len(g.blocks()) == 10 and len({b[:2] for b in g.blocks()}) == 2
        assert all(c.kmers[-1] < 1 << K2 and all(y > x for x, y in zip(c.kmers, c.kmers[1:])) for c in cases)
    c, nbytes = db.launches_case(21)
    assert nbytes >= 1300000 and set(c.blocks()) == {(42, 22, db.BLOCK)} and len(c.blocks()) == 40


@pytest.mark.parametrize("k", [21, 30, 31])
def test_the_placed_catalogue_holds_every_class_it_names(k, tmp_path):
    """the placed kernel's files, cut from a library-written placed file: every last-block length behind a full block, one record, two-record
    last blocks at kbits 0 / 1 / 2, one jump of 2^40 or more at each seam among differences a sixteenth of it at most, ten blocks of
    alternating widths -- each a placed file that the host reader converts back to the k-mers and counts it was cut from"""
    m = _m()
    r = np.random.default_rng(800 + k)
    special = [x for pair in db.twins(k, r, 3) + db.window_neighbours(k, r, 3) for x in pair]
    km = np.union1d(canon(r, k, 70000), np.array(special, dtype=np.uint64))
    vals = (1 + (km % np.uint64(300))).astype(np.uint32)
    vals[1::53] = (1 << 21) - 1
    vals[2::59] = 1 << 22
    src = db.placed_source(m, k, km, vals, str(tmp_path / "src"))
    big = db.placed_big(k)
    assert big >= 1 << 40
    cuts = db.placed_cuts(k, src.records, src.kmers, big)
    seen = {}
    for name, idx, widths in cuts:
        path, back = db.write_cut(str(tmp_path / (name + ".mfxk")), src, idx, widths), str(tmp_path / (name + ".back"))
        assert m.db_probe(path).get("placed") and m.db_convert(path, back) == len(idx), name
        kk, keys, cnts = db.decode_delta(back)
        want = sorted((src.kmers[i], src.counts[i]) for i in idx)
        assert kk == k and list(zip(keys, cnts)) == want, name
        raw = db.decode_raw(path)
        seen[name] = [(kb, vb, min(db.BLOCK, len(idx) - b * db.BLOCK)) for b, (kb, vb) in enumerate(raw.widths)], raw.records
    for L in db.LENGTHS:
        assert [b[2] for b in seen["len%d" % L][0]] == [db.BLOCK, L]
    assert seen["len1"][0][1][0] == 0 and [b[2] for b in seen["n1"][0]] == [1]
    assert [b[0::2] for b in seen["twins"][0]][1] == (0 if k == 31 else 1, 2)
    assert [b[0::2] for b in seen["neighbours"][0]][1] == (1 if k == 31 else 2, 2)
    blocks, rec = seen["carry"]
    assert len(blocks) == len(db.PLACED_CARRY_ENTRIES) and {b[2] for b in blocks} == {db.BLOCK}
    for b, e in enumerate(db.PLACED_CARRY_ENTRIES):
        d = [y - x for x, y in zip(rec[b * db.BLOCK:], rec[b * db.BLOCK + 1:(b + 1) * db.BLOCK])]
        assert d[e - 1] >= big and sorted(d)[-2] <= big >> 4, (k, e)
    assert {255, 256, 1023, 1024} <= set(db.PLACED_CARRY_ENTRIES)     # a wave's and a round's seam, from both sides
    blocks, rec = seen["grid"]
    rec_bits = 64 if k == 31 else 2 * k + 3
    assert len(blocks) == 10 and all(b[0] == rec_bits and b[1] == 22 for b in blocks[1::2]) and all(b[0] < rec_bits for b in blocks[0::2])
    assert all(rec[(b + 1) * db.BLOCK] - rec[(b + 1) * db.BLOCK - 1] >= big for b in range(9))


def test_a_placed_31mer_file_with_a_64_bit_difference_converts_back(tmp_path):
    """k = 31: the stored number of a placed record has 64 bits, so two neighbouring records of a block can lie 2^63 or more apart and
    the writer then takes kbits = 64.  Every reader must take that width: placed -> sorted gives back the k-mers and counts.  (Only a
    database of two or three k-mers can have such a gap: about one random pair in four.)"""
    m = _m()
    k = 31
    found = 0
    for seed in range(64):
        r = np.random.default_rng(7000 + seed)
        km = canon(r, k, 2 + seed % 2)
        if len(km) < 2:
            continue
        vals = np.array([5, (1 << 21) + 1, 70000][:len(km)], dtype=np.uint32)
        flat, placed, back = (str(tmp_path / x) for x in ("f.mfxk", "p.mfxk", "b.mfxk"))
        m.db_write_flat(flat, k, km, vals)
        assert m.db_convert_placed(flat, placed) == len(km)
        raw = db.decode_raw(placed)
        if max(y - x for x, y in zip(raw.records, raw.records[1:])) < 1 << 63:
            continue
        found += 1
        assert raw.widths[0][0] == 64
        assert m.db_convert(placed, back) == len(km)
        kk, keys, cnts = db.decode_delta(back)
        assert kk == k and keys == km.tolist() and cnts == vals.tolist()
        if found == 4:
            break
    assert found == 4                                          # (the search is seeded: the same files every run)
