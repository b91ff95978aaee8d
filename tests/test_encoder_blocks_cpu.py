"""The writers' catalogue (tests/encoder_blocks.py) on the reference alone, and through the two HOST writers.  What is asserted here is what
keeps tests/test_gpu_encoder_blocks.py from being vacuous: the Python rule (delta_blocks.plan_widths) names, for every block of every world,
the (kbits, vbits) and the number of escapes the block was built for; every kbits 1 .. 62 and every vbits 2 .. 22 occurs in a FULL block
(the only ones the device encodes); the word-boundary classes, the cost edges and the escape positions occur.  Then mfx_db_write_flat and
DbWriter(streamed=True).append_sorted give the Python encoder's bytes for every world, so the expected bytes rest on two independent
implementations.  No device."""
import os

import numpy as np
import pytest

from tests import delta_blocks as db
from tests import encoder_blocks as eb

BLOCK = eb.BLOCK


def _vbin(c):
    return (int(c) + 1).bit_length()


def _cost(counts, vb):
    return len(counts) * vb + 96 * sum(c >= (1 << vb) - 1 for c in counts)


@pytest.mark.parametrize("name", eb.names())
def test_every_block_is_what_it_is_named(name):
    w = eb.world(name)
    kmers, counts = w.kmers.tolist(), w.counts.tolist()
    assert w.k == 31 and kmers[-1] < 4 ** 31 and min(counts) >= 1
    assert sum(b.n for b in w.blocks) == len(kmers) and all(b.n == BLOCK for b in w.blocks[:-1]) and 0 < w.blocks[-1].n < BLOCK
    plan = db.plan_widths(kmers, counts, None)
    assert len(plan) == len(w.blocks)
    for i, (b, (kb, vb)) in enumerate(zip(w.blocks, plan)):
        c = counts[i * BLOCK:(i + 1) * BLOCK]
        escapes = [j for j, x in enumerate(c) if x >= (1 << vb) - 1]
        assert (kb, vb, len(escapes)) == (b.kb, b.vb, b.nesc), (name, i, b.label)
        assert escapes == b.esc_at, (name, i, b.label)
        if b.n == BLOCK and b.nesc < BLOCK:
            assert (1 << vb) - 2 in c, (name, i)                   # the largest count the field holds
    eb.expected_bytes(w)
    assert [tuple(x) for x in w.written] == [(b.kb, b.vb) for b in w.blocks]             # ... and the widths the encoder wrote


def test_the_catalogue_holds_every_width_and_class():
    full = [(w, i, b) for w in eb.worlds() for i, b in enumerate(w.blocks) if b.n == BLOCK]
    assert {b.kb for _, _, b in full} == set(range(1, 63))
    assert {b.vb for _, _, b in full} == set(range(2, 23))
    pairs = {}
    for _, _, b in full:
        pairs.setdefault(b.kb, set()).add(b.vb)
    assert all(len(pairs[kb]) >= 2 for kb in range(1, 63))         # every kbits beside two different vbits
    # the decoder catalogue's word-boundary classes: a field ends on a boundary, crosses it by one bit, a last field crosses into the last word
    assert db.straddles([(b.kb, b.vb, b.n) for _, _, b in full]) == (True, True, True)
    # full-width differences where the word assembly can lose them: the first field, the last, one that crosses a word boundary
    for w in eb.worlds():
        if w.name not in ("kb_up", "kb_down"):
            continue
        keys = w.kmers.tolist()
        for i, b in enumerate(w.full()):
            k = keys[i * BLOCK:(i + 1) * BLOCK]
            d = [y - x for x, y in zip(k, k[1:])]
            assert d[0].bit_length() == b.kb and d[BLOCK - 2].bit_length() == b.kb
            crossing = [j for j in range(BLOCK - 1) if (j * b.kb) % 64 + b.kb > 64]
            assert (64 % b.kb == 0 and not crossing) or any(d[j].bit_length() == b.kb for j in crossing), b.kb
            if crossing:                                           # ... one with the fewest bits behind the boundary, one with the fewest in front
                behind, front = min((j * b.kb) % 64 + b.kb - 64 for j in crossing), min(64 - (j * b.kb) % 64 for j in crossing)
                assert any(d[j].bit_length() == b.kb and (j * b.kb) % 64 + b.kb - 64 == behind for j in crossing), b.kb
                assert any(d[j].bit_length() == b.kb and 64 - (j * b.kb) % 64 == front for j in crossing), b.kb
            assert sorted(d)[-5].bit_length() <= min(b.kb, 40)     # the others: at most 40 bits
    # 57 bits and more: as many full-width differences as 4^31 leaves; 62 bits: one of 2^61 or more, and the largest 31-mer ends a file
    many = {}
    for w, i, b in full:
        if b.kb >= 57:
            k = w.kmers.tolist()[i * BLOCK:(i + 1) * BLOCK]
            many.setdefault(b.kb, set()).add(sum((y - x).bit_length() == b.kb for x, y in zip(k, k[1:])))
    assert many == {57: {8}, 58: {4}, 59: {2}, 60: {1}, 61: {1}, 62: {1}}
    assert int(eb.world("kb62a").kmers[-1]) == 4 ** 31 - 1 and int(eb.world("kb_up").kmers[0]) == 0


def test_the_cost_edges_are_edges():
    """42 escapes are cheaper than one bit more for 4096 fields, 43 are not; 128 x 96 = 3 x 4096 and 256 x 96 = 6 x 4096 are ties"""
    w = eb.world("cost_edges")
    counts = w.counts.tolist()
    seen = {}
    for i, b in enumerate(w.full()):
        c = counts[i * BLOCK:(i + 1) * BLOCK]
        seen.setdefault(b.label, []).append(b.vb)
        if b.label == "stay42":
            assert b.nesc == 42 and all(_vbin(c[j]) == b.vb + 1 for j in b.esc_at) and _cost(c, b.vb) + 64 == _cost(c, b.vb + 1)
        elif b.label == "widen43":
            assert b.nesc == 0 and sum(_vbin(x) == b.vb for x in c) == 43 and _cost(c, b.vb - 1) == _cost(c, b.vb) + 32
        elif b.label == "tie128":
            assert b.nesc == 128 and all(_vbin(c[j]) == b.vb + 3 for j in b.esc_at) and _cost(c, b.vb) == _cost(c, b.vb + 3)
        elif b.label == "tie256":
            assert b.nesc == 256 and all(_vbin(c[j]) == b.vb + 6 for j in b.esc_at) and _cost(c, b.vb) == _cost(c, b.vb + 6)
        elif b.label == "all_escape":
            assert (b.vb, b.nesc) == (2, BLOCK) and min(c) >= 2**22 - 1 and 2**32 - 1 in c
        elif b.label == "vb22":
            assert b.vb == 22 and {2**22 - 2, 2**22 - 1, 2**32 - 1} <= set(c) and _vbin(2**32 - 1) == 33
    assert {k: len(set(v)) for k, v in seen.items()} == {"stay42": 3, "widen43": 3, "tie128": 3, "tie256": 3, "all_escape": 1, "vb22": 1}
    assert 21 in seen["stay42"] and 22 in seen["widen43"] and 19 in seen["tie128"] and 16 in seen["tie256"]      # up to the widest field


def test_the_escape_positions_occur():
    w = eb.world("escape_positions")
    counts = w.counts.tolist()
    full = w.full()
    at = [b.esc_at for b in full]
    assert [0] in at and [4095] in at and [63, 64] in at and [255, 256, 257] in at
    runs = [(i, b) for i, b in enumerate(full) if b.label == "run300"]
    assert len(runs) == 2
    for i, b in runs:
        c = counts[i * BLOCK:(i + 1) * BLOCK]
        assert b.nesc == 300 and b.esc_at == list(range(b.esc_at[0], b.esc_at[0] + 300)) and all(c[j] == 2**32 - 1 for j in b.esc_at)
        assert b.esc_at[0] // 256 != b.esc_at[-1] // 256           # across the end of a round of 256 lanes
        assert db.writer_vbits([x for j, x in enumerate(c) if j not in set(b.esc_at)]) == b.vb      # they did not move vbits
    none_between = [i for i in range(1, len(full) - 1) if full[i].nesc == 0 and full[i - 1].nesc and full[i + 1].nesc]
    assert len(none_between) >= 3
    # (the key-width files: every tenth block without an escape)
    assert sum(b.nesc == 0 for b in eb.world("kb_up").full()) >= 5


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", eb.names())
def test_host_writers_give_the_python_encoders_bytes(tmp_path, name):
    import merfin_amd as m
    w = eb.world(name)
    want = eb.expected_bytes(w)
    out = str(tmp_path / "flat.mfxk")
    m.db_write_flat(out, w.k, w.kmers, w.counts)
    assert _read(out) == want
    out = str(tmp_path / "streamed.mfxk")
    wr = m.DbWriter(out, w.k, streamed=True)
    n, lo, step = len(w.kmers), 0, 0
    sizes = (1, 4095, 4097, 3, 2 * 4096, 5000, 12345)              # uneven slices: carries of every kind in front of the full blocks
    while lo < n:
        hi = min(n, lo + sizes[step % len(sizes)])
        assert wr.append_sorted(w.kmers[lo:hi], w.counts[lo:hi]) == hi - lo
        lo, step = hi, step + 1
    assert wr.close() == n and not os.path.exists(out + ".blocks")
    assert _read(out) == want
    # and the Python decoder reads the arrays back from those bytes
    k, keys, vals = db.decode_delta(out)
    assert k == w.k and np.array_equal(np.array(keys, dtype=np.uint64), w.kmers) and np.array_equal(np.array(vals, dtype=np.uint32), w.counts)
