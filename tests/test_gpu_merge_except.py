"""db_merge_except / mfx_db_merge_except: db_merge over the inputs without the k-mers that a subtracted database holds, whatever its count
there.  The file's bytes equal db_write_flat of the numpy result: the operation over the inputs (tests/test_gpu_merge.py: reference), then
~np.isin(k-mers, union of the subtracted), then the filter on the combined count."""
import os

import numpy as np
import pytest

from tests import stream_worlds as sw
from tests.test_gpu_merge import OPS, TOP, _bytes, _write, reference

pytestmark = pytest.mark.gpu

K = 21
SIZES = (0, 1, 4095, 4096, 4097, 20000)
FILTERS = ((0, TOP), (2, TOP), (0, 1))                        # none, -min 2, -max 1


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def expected(inputs, nots, op, lo=0, hi=TOP):
    """(k-mers, counts, n_filtered, n_subtracted)"""
    rk, rv, _, _ = reference(inputs, op)                      # what the operation yields, unfiltered
    barred = np.isin(rk, np.concatenate([a for a, _ in nots]).astype(np.uint64)) if nots else np.zeros(len(rk), dtype=bool)
    inside = (rv.astype(np.uint64) >= lo) & (rv.astype(np.uint64) <= hi)
    keep = ~barred & inside
    return rk[keep], rv[keep], int((~barred & ~inside).sum()), int(barred.sum())


def check(m, tmp_path, inputs, nots, op, lo=0, hi=TOP, tag="x", k=K):
    paths = [_write(m, tmp_path / ("%s_in%d.mfxk" % (tag, i)), k, a, b) for i, (a, b) in enumerate(inputs)]
    npaths = [_write(m, tmp_path / ("%s_not%d.mfxk" % (tag, i)), k, a, b) for i, (a, b) in enumerate(nots)]
    before = [_bytes(p) for p in paths + npaths]
    rk, rv, nfilt, nsub = expected(inputs, nots, op, lo, hi)
    want = _bytes(_write(m, tmp_path / (tag + "_want.mfxk"), k, rk, rv))
    out = str(tmp_path / (tag + "_out.mfxk"))
    st = m.db_merge_except(paths, npaths, out, op=op, min_count=lo, max_count=hi)
    assert not os.path.exists(out + ".blocks")
    assert _bytes(out) == want, (op, lo, hi, [len(a) for a, _ in inputs], [len(a) for a, _ in nots], st)
    assert (st["n_in"], st["n_out"], st["n_filtered"], st["n_subtracted"]) == (sum(len(a) for a, _ in inputs), len(rk), nfilt, nsub), st
    assert [_bytes(p) for p in paths + npaths] == before
    return st, out, paths


def _sets(sizes, seed):
    """databases of these sizes drawn from one pool, so that they share k-mers; counts 1 to 4"""
    rng = np.random.default_rng(seed)
    pool = sw.random_keys(K, 30000, seed)
    out = []
    for n in sizes:
        keys = np.sort(rng.choice(pool, size=n, replace=False)) if n else np.zeros(0, dtype=np.uint64)
        out.append((keys.astype(np.uint64), rng.integers(1, 5, size=n).astype(np.uint32)))
    return out


@pytest.mark.parametrize("n_not", [0, 1, 2])
@pytest.mark.parametrize("n_in", [1, 2, 3])
def test_inputs_nots_ops_and_filters(tmp_path, monkeypatch, n_in, n_not):
    m = _mfx()
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")             # several windows
    at = 3 * n_in + n_not                                     # every size of the list is an input and a subtracted database somewhere
    sets = _sets([SIZES[(at + i) % 6] if i else 20000 for i in range(n_in)] + [SIZES[(at + 2 * j + 1) % 6] for j in range(n_not)], 100 + at)
    inputs, nots = sets[:n_in], sets[n_in:]
    for op in OPS:
        for f, (lo, hi) in enumerate(FILTERS):
            st, out, paths = check(m, tmp_path, inputs, nots, op, lo, hi, tag="%s%d" % (op, f))
            assert st["windows"] > 1
            if n_not == 0:                                    # no subtracted database: db_merge, byte for byte
                plain = str(tmp_path / "plain.mfxk")
                m.db_merge(paths, plain, op=op, min_count=lo, max_count=hi)
                assert _bytes(plain) == _bytes(out)


@pytest.mark.parametrize("size", SIZES)
def test_every_size_as_input_and_as_subtracted(tmp_path, monkeypatch, size):
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    big, small = _sets([20000, size], 200 + size)
    check(m, tmp_path, [big], [small], "sum", tag="a")
    check(m, tmp_path, [small], [big], "sum", tag="b")
    check(m, tmp_path, [small, big], [small], "intersect", tag="c")


@pytest.mark.parametrize("rng", [None, "1"])
def test_subtracted_kmers_on_block_and_window_edges(tmp_path, monkeypatch, rng):
    """the first and the last k-mer of a block, of a window (MFX_MERGE_RANGE=1: a window a block) and of the file are subtracted"""
    m = _mfx()
    if rng:
        monkeypatch.setenv("MFX_MERGE_RANGE", rng)
    else:
        monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    a = sw.random_keys(K, 2 * 4096 + 10, 31)
    av = np.full(len(a), 3, dtype=np.uint32)
    edges = a[[0, 4095, 4096, 8191, 8192, len(a) - 1]]
    st, _, _ = check(m, tmp_path, [(a, av)], [(edges, np.ones(len(edges), dtype=np.uint32))], "sum")
    assert st["n_subtracted"] == 6 and (rng is None or st["windows"] >= 3)
    # a subtracted database that holds k-mers below, between and above the input's, and none of them
    other = np.setdiff1d(sw.random_keys(K, 5000, 32), a)
    st, _, _ = check(m, tmp_path, [(a, av)], [(other, np.ones(len(other), dtype=np.uint32))], "max", tag="y")
    assert st["n_subtracted"] == 0 and st["n_out"] == len(a)


def test_the_input_itself_and_an_empty_database(tmp_path):
    m = _mfx()
    (a, av), (b, bv) = _sets([4097, 4095], 41)
    empty = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    # a subtracted database equal to the input: a valid file of no k-mers
    st, out, paths = check(m, tmp_path, [(a, av)], [(a, av)], "sum", tag="self")
    assert st["n_out"] == 0 and st["n_subtracted"] == len(a) and m.db_probe(out)["n_kmers"] == 0
    st2 = m.db_merge_except(paths, paths, str(tmp_path / "same_file.mfxk"))      # ... and the input's own file
    assert st2["n_out"] == 0 and _bytes(str(tmp_path / "same_file.mfxk")) == _bytes(out)
    # an empty subtracted database subtracts nothing
    st, out, paths = check(m, tmp_path, [(a, av), (b, bv)], [empty], "sum", tag="none")
    plain = str(tmp_path / "plain.mfxk")
    m.db_merge(paths, plain)
    assert st["n_subtracted"] == 0 and _bytes(plain) == _bytes(out)
    check(m, tmp_path, [empty], [(a, av)], "sum", tag="of_nothing")


def test_escaped_counts(tmp_path):
    """a subtracted k-mer whose count there needs an escape; an input count that needs one and survives"""
    m = _mfx()
    a = sw.random_keys(K, 5000, 51)
    av = np.full(len(a), 2, dtype=np.uint32)
    av[[10, 4096, 4999]] = [2**22 - 1, 2**32 - 1, 2**31]     # escapes in the input: the second is subtracted, the others survive
    nk = a[[7, 4096, 4500]]
    nv = np.array([2**32 - 1, 5, 2**22 - 1], dtype=np.uint32)  # escapes in the subtracted database
    for op in OPS:
        st, out, _ = check(m, tmp_path, [(a, av)], [(nk, nv)], op, tag=op)
        assert st["n_subtracted"] == 3
    ix = m.Index(K, 6000)
    ix.load_db(out, 0)
    ek, er, _ = ix.export()
    assert len(ek) == len(a) - 3 and int(er[ek == a[10]][0]) == 2**22 - 1 and int(er[ek == a[4999]][0]) == 2**31 and not np.isin(nk, ek).any()


def test_refusals_leave_nothing(tmp_path):
    m = _mfx()
    (a, av), (b, bv) = _sets([100, 50], 61)
    pa, pb = _write(m, tmp_path / "a.mfxk", K, a, av), _write(m, tmp_path / "b.mfxk", K, b, bv)
    out = str(tmp_path / "out.mfxk")
    p15 = _write(m, tmp_path / "c.mfxk", 15, np.array([1, 2], dtype=np.uint64), np.array([1, 1], dtype=np.uint32))
    with pytest.raises(m.MfxError) as e:
        m.db_merge_except([pa], [p15], out)
    assert "of one k" in str(e.value) and not os.path.exists(out)
    with pytest.raises(m.MfxError) as e:
        m.db_merge_except([pa] * 40, [pb] * 25, out)
    assert "64" in str(e.value) and not os.path.exists(out)
    before = _bytes(pb)
    with pytest.raises(m.MfxError) as e:
        m.db_merge_except([pa], [pb], pb)
    assert "is the subtracted database" in str(e.value) and _bytes(pb) == before
    with pytest.raises(m.MfxError):
        m.db_merge_except([pa], [str(tmp_path / "gone.mfxk")], out)
    assert not os.path.exists(out)
    with pytest.raises(m.MfxError):                           # the operations stay four
        m.db_merge_except([pa], [pb], out, op=4)
    assert m.db_merge_except([pa] * 40, [pb] * 24, out)["n_out"] == int((~np.isin(a, b)).sum())
