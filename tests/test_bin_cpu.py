"""The host arithmetic of -bin (csrc/mfx_bin.h) through mfx_bin_plan_host and mfx_bin_classify: the pieces records are cut into by the
batcher the device path shares with the read counters, and the class rule against the Python integers of tests/bin_ref.py.  No device."""
import itertools

import numpy as np
import pytest

from tests import bin_ref as br


def _mfx():
    import merfin_amd as m
    return m


def lens_grid(k):
    return [0, k - 1, k, k + 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 5]


def check_plan(m, lens, k, batch):
    """the invariants of the cut; returns the plan"""
    p = m.bin_plan_host(lens, k, batch)
    assert p.dtype == np.uint64 and p.shape[1] == 4
    cap = batch or (1 << 26)
    kmers = [0] * len(lens)
    batches_of = [[] for _ in lens]
    last = None
    for b, r, first, n in p.tolist():
        assert n >= k, (b, r, first, n)                              # no piece is shorter than k
        assert first + n <= cap
        kmers[r] += max(0, n - k + 1)
        batches_of[r].append(b)
        if last is not None:
            lb, lr, lend = last
            assert (b, r) >= (lb, lr)                                # input order
            if b == lb:
                assert first == lend + 1, (b, r)                     # pieces ascend within a batch, one separator between two
                assert r > lr
            else:
                assert b == lb + 1 and first == 0                    # batches are numbered as they fill
        else:
            assert b == 0 and first == 0
        last = (b, r, first + n)
    for r, n in enumerate(lens):
        assert kmers[r] == max(0, n - k + 1), (r, n)                 # every k-mer of a record lies in exactly one piece
        bs = batches_of[r]
        assert bs == list(range(bs[0], bs[0] + len(bs))) if bs else n < k      # ... and its pieces in consecutive batches
    return p


@pytest.mark.parametrize("k", [6, 21, 31])
def test_plan_over_the_length_grid(k):
    m = _mfx()
    grid = lens_grid(k)
    for batch in (2 * k + 2, 100, 4096, 10000):
        if batch < 2 * k + 2:
            continue
        check_plan(m, grid, k, batch)
        check_plan(m, grid[::-1], k, batch)
        check_plan(m, grid * 3, k, batch)
        for n in grid:
            check_plan(m, [n], k, batch)
        for a, b in itertools.product(grid[:5], repeat=2):
            check_plan(m, [a, b, a], k, batch)


def test_plan_shapes():
    m = _mfx()
    k = 21
    # a record that ends exactly at a batch's end: no separator, the next record opens the next batch
    p = check_plan(m, [60, 39, 50], k, 100)
    assert p.tolist() == [[0, 0, 0, 60], [0, 1, 61, 39], [1, 2, 0, 50]]
    # less than k bases of room: the batch goes before the record is cut into it
    p = check_plan(m, [70, 50], k, 100)
    assert p.tolist() == [[0, 0, 0, 70], [0, 1, 71, 29], [1, 1, 0, 41]]
    p = check_plan(m, [80, 50], k, 100)
    assert p.tolist() == [[0, 0, 0, 80], [1, 1, 0, 50]]
    # a record across many batches of the smallest size: every piece but the last fills its batch
    p = check_plan(m, [1000], k, 2 * k + 2)
    assert len(p) > 40 and set(p[:-1, 3].tolist()) == {2 * k + 2} and set(p[:, 2].tolist()) == {0}
    # all-short record lists: no piece
    assert len(check_plan(m, [0, 1, k - 1, 5, 0], k, 100)) == 0
    assert len(check_plan(m, [], k, 100)) == 0
    # the default batch
    p = check_plan(m, [100, 30000], k, 0)
    assert p.tolist() == [[0, 0, 0, 100], [0, 1, 101, 30000]]


def test_plan_random_lengths():
    m = _mfx()
    r = np.random.default_rng(11)
    for k, batch in ((6, 14), (15, 100), (21, 4096), (31, 64), (21, 10000)):
        lens = np.where(r.random(400) < 0.3, r.integers(0, k + 3, 400), r.integers(0, 3 * batch, 400))
        check_plan(m, lens.tolist(), k, batch)


def test_plan_refusals():
    m = _mfx()
    for k, batch in ((21, 43), (21, 1), (0, 100), (65, 1000), (21, (1 << 34) + 1)):
        with pytest.raises(m.MfxError) as e:
            m.bin_plan_host([100], k, batch)
        assert e.value.code == -1


def test_classify_against_python_integers():
    m = _mfx()
    big = 2**32 - 1
    vals = [0, 1, 2, 3, 4, 5, 9, 10, 25, 1000, 2499, 2500, 2501, big - 1, big]
    norms = [(0, 0), (1, 1), (100, 100), (100, 250), (250, 100), (7, 3), (4**31 - 1, 4**31 - 1), (4**31 - 1, 1), (1, 4**31 - 1), (4**31 - 1, 4**31 - 2)]
    rows = np.array([[a + b, a, b, 0] for a in vals for b in vals if a + b <= big] + [[big, big, 0, 0], [big, 0, big, 0]], dtype=np.uint32)
    seen = set()
    for (na, nb), ratio, hits in itertools.product(norms, (1000, 1001, 2500), (0, 1, 2, 5, 10, 11, big)):
        got = m.bin_classify(rows, na, nb, ratio, hits)
        want = br.classes(rows.tolist(), na, nb, ratio, hits)
        assert got.dtype == np.uint8 and got.tolist() == want, (na, nb, ratio, hits)
        seen |= set(want)
    assert seen == {0, 1, 2}
    # ties and zeros are unknown whatever the options; the 128-bit product decides the largest operands
    assert m.bin_classify([[0, 0, 0, 0], [8, 4, 4, 0]], 5, 5, 1000, 0).tolist() == [2, 2]
    top = 4**31 - 1
    assert m.bin_classify([[0, big, big - 1, 0], [0, big - 1, big, 0], [0, big, big, 0]], top, top).tolist() == [0, 1, 2]
    assert m.bin_classify([[0, big, big, 0]], top, top - 1).tolist() == [1]
    assert br.classify(big, big - 1, top, top) == 0 and br.classify(big - 1, big, top, top) == 1 and br.classify(big, big, top, top) == 2
    assert br.classify(big, big, top, top - 1) == 1              # a = b, set B smaller: B's share is larger
    # min_hits edges
    assert m.bin_classify([[9, 2, 1, 0]], 1, 1, 1000, 3).tolist() == [0] and m.bin_classify([[9, 2, 1, 0]], 1, 1, 1000, 4).tolist() == [2]
    # ratio edges: a = 2.5 b is no A at 2500, is at 1000 and 1001 * b < 1000 * a
    assert m.bin_classify([[0, 2500, 1000, 0], [0, 2501, 1000, 0], [0, 1001, 1000, 0], [0, 1002, 1000, 0]], 1, 1, 2500, 1).tolist() == [2, 0, 2, 2]
    assert m.bin_classify([[0, 1001, 1000, 0], [0, 1002, 1000, 0]], 1, 1, 1001, 1).tolist() == [2, 0]
    with pytest.raises(m.MfxError) as e:
        m.bin_classify(rows, 1, 1, 999, 1)
    assert e.value.code == -1 and "ratio" in str(e.value)
    assert len(m.bin_classify(np.zeros((0, 4), dtype=np.uint32), 1, 1)) == 0
