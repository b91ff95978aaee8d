"""mfx_db_merge on the device (csrc/mfx_merge.hip: decode, merge path, combine; csrc/mfx_db_merge.cpp: the windows' driver and the streamed
writer behind it).  Every result is compared byte for byte with mfx_db_write_flat of a numpy reference -- the inputs concatenated,
np.unique with its inverse, np.add.at in 64 bits then clipped (np.maximum.at / np.minimum.at; presence counts for intersect), then the
filter -- and loaded back through the table's decode kernel.  The sizes are the smallest at which the code can go wrong: inputs of 0, 1 and
around one block of 4096 k-mers up to three blocks and a piece, windows (MFX_MERGE_RANGE) of everything, about a quarter block, and one
block first k-mer each."""
import os

import numpy as np
import pytest

from tests import stream_worlds as sw

pytestmark = pytest.mark.gpu

OPS = ("sum", "max", "min", "intersect")
TOP = 2**32 - 1
SIZES = (0, 1, 4095, 4096, 4097, 3 * 4096 + 5)
_cache = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def reference(inputs, op, lo=0, hi=TOP):
    """(k-mers, counts, n_filtered, n_saturated) of the merge of [(k-mers, counts)]"""
    keys = np.concatenate([a for a, _ in inputs]).astype(np.uint64)
    vals = np.concatenate([b for _, b in inputs]).astype(np.uint64)
    if len(keys) == 0:
        return keys, vals.astype(np.uint32), 0, 0
    u, inv = np.unique(keys, return_inverse=True)
    sat = 0
    if op == "sum":
        c = np.zeros(len(u), dtype=np.uint64)
        np.add.at(c, inv, vals)
        sat = int((c > TOP).sum())
        c = np.minimum(c, np.uint64(TOP))
    elif op == "max":
        c = np.zeros(len(u), dtype=np.uint64)
        np.maximum.at(c, inv, vals)
    else:
        c = np.full(len(u), TOP, dtype=np.uint64)
        np.minimum.at(c, inv, vals)
    yields = np.ones(len(u), dtype=bool)
    if op == "intersect":
        yields = np.bincount(inv, minlength=len(u)) == len(inputs)
    keep = yields & (c >= lo) & (c <= hi)
    return u[keep], c[keep].astype(np.uint32), int((yields & ~keep).sum()), sat


def _write(m, path, k, keys, vals):
    m.db_write_flat(str(path), k, np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(vals, dtype=np.uint32))
    return str(path)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _check(m, tmp_path, k, inputs, op, lo=0, hi=TOP, load_back=True, tag="x"):
    """one merge against the reference: the bytes, the stats, no spool, the inputs unchanged, the file through the decode kernel"""
    paths = [_write(m, tmp_path / ("%s_in%d.mfxk" % (tag, i)), k, a, b) for i, (a, b) in enumerate(inputs)]
    return check_paths(m, tmp_path, k, paths, inputs, op, lo, hi, load_back, tag)


def check_paths(m, tmp_path, k, paths, inputs, op, lo=0, hi=TOP, load_back=True, tag="x"):
    """... of input files that exist, whoever wrote them: paths[i] holds the arrays inputs[i]"""
    before = [_bytes(p) for p in paths]
    rk, rv, nfilt, nsat = reference(inputs, op, lo, hi)
    want = _bytes(_write(m, tmp_path / (tag + "_want.mfxk"), k, rk, rv))
    out = str(tmp_path / (tag + "_out.mfxk"))
    st = m.db_merge(paths, out, op=op, min_count=lo, max_count=hi)
    assert not os.path.exists(out + ".blocks")
    assert _bytes(out) == want, (k, op, lo, hi, [len(a) for a, _ in inputs], st)
    assert (st["n_in"], st["n_out"], st["n_filtered"], st["n_saturated"]) == (sum(len(a) for a, _ in inputs), len(rk), nfilt, nsat), st
    assert [_bytes(p) for p in paths] == before
    if load_back and len(rk):
        ix = m.Index(k, len(rk) + 64)
        ix.load_db(out, 0)
        ek, er, ea = ix.export()
        np.testing.assert_array_equal(ek, rk)
        np.testing.assert_array_equal(er, rv)
        assert not ea.any()
    return st


def _world(k, relation, sizes, seed=0):
    """inputs of the given sizes (clipped to the key space) that are disjoint, identical, interleaved or nested"""
    key = (k, relation, tuple(sizes), seed)
    if key in _cache:
        return _cache[key]
    space = 4 ** k
    sizes = [min(s, space // 2) for s in sizes]
    rng = np.random.default_rng(1000 * k + seed)
    out = []
    if relation == "disjoint":                                     # one key set dealt out at random: no key twice, the inputs' ranges overlap
        pool = sw.random_keys(k, sum(sizes), 11 + seed)
        perm = rng.permutation(len(pool))
        at = 0
        for s in sizes:
            out.append(np.sort(pool[perm[at:at + s]]))
            at += s
    elif relation == "identical":
        keys = sw.random_keys(k, max(sizes), 12 + seed)
        out = [keys for _ in sizes]
    elif relation == "interleaved":                                # every input its own draw from a pool twice the largest: about half of it shared
        pool = sw.random_keys(k, min(2 * max(max(sizes), 1), space), 13 + seed)
        out = [np.sort(rng.choice(pool, size=s, replace=False)) for s in sizes]
    else:                                                          # nested: every input a subset of the one before it
        keys = sw.random_keys(k, max(sizes), 14 + seed)
        for s in sorted(sizes, reverse=True):
            keys = np.sort(rng.choice(keys, size=s, replace=False))
            out.append(keys)
    _cache[key] = [(a, sw.mixed_counts(len(a), 7 * i + seed)) for i, a in enumerate(out)]
    return _cache[key]


def _shape_cases():
    out = []
    rel = ("disjoint", "identical", "interleaved", "nested")
    plans = [(1, (SIZES[5],)), (2, (SIZES[3], SIZES[4])), (3, (SIZES[2], SIZES[5], SIZES[1])), (5, (SIZES[4], SIZES[0], SIZES[2], SIZES[1], SIZES[3])),
             (2, (SIZES[0], SIZES[0])), (2, (SIZES[1], SIZES[5]))]
    for ki, k in enumerate((7, 15, 21, 31)):
        for ri, r in enumerate(rel):
            n_in, sizes = plans[(ki + ri) % len(plans)]
            out.append(pytest.param(k, r, sizes, id="k%d-%s-%s" % (k, r, "_".join(map(str, sizes)))))
        n_in, sizes = plans[(ki + 4) % len(plans)]
        out.append(pytest.param(k, "interleaved", sizes, id="k%d-interleaved-%s" % (k, "_".join(map(str, sizes)))))
        n_in, sizes = plans[(ki + 5) % len(plans)]
        out.append(pytest.param(k, "disjoint", sizes, id="k%d-disjoint-%s" % (k, "_".join(map(str, sizes)))))
    return out


@pytest.mark.parametrize("k,relation,sizes", _shape_cases())
def test_sizes_and_shapes(tmp_path, monkeypatch, k, relation, sizes):
    m = _mfx()
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    inputs = _world(k, relation, sizes)
    for op in OPS:
        st = _check(m, tmp_path, k, inputs, op, tag=op)
        assert st["windows"] == (1 if sum(len(a) for a, _ in inputs) else 0)


def test_sixty_four_tiny_inputs(tmp_path):
    m = _mfx()
    rng = np.random.default_rng(64)
    inputs = []
    for i in range(64):
        keys = np.unique(rng.integers(0, 4 ** 9, size=40 + i, dtype=np.uint64))
        keys = np.union1d(keys, np.array([5, 77777], dtype=np.uint64))        # two k-mers every input holds
        inputs.append((keys, sw.mixed_counts(len(keys), i)))
    for op in OPS:
        _check(m, tmp_path, 9, inputs, op, tag=op)


@pytest.mark.parametrize("name", ["all7mers", "pair62"])
def test_block_widths(tmp_path, name):
    """kb = 1 (every 7-mer, against itself) and kb = 62 (the smallest and the largest 31-mer)"""
    m = _mfx()
    k, keys, vals = sw.all_7mers() if name == "all7mers" else sw.pair62()
    other = (keys, sw.mixed_counts(len(keys), 99)) if name == "all7mers" else (np.array([1, 2**62 - 1], dtype=np.uint64), np.array([7, 9], dtype=np.uint32))
    for op in OPS:
        _check(m, tmp_path, k, [(keys, vals), other], op, tag=op)
    _check(m, tmp_path, k, [(keys, vals)], "sum", tag="alone")


def test_escapes_in_and_out(tmp_path):
    """counts of 2^22 - 2 (the widest field), 2^22 - 1 and 2^32 - 1 (escapes) in the inputs; sums that newly cross 2^22 - 1; the clamp"""
    m = _mfx()
    k = 21
    keys = sw.random_keys(k, 4096 + 300, 5)
    a = np.full(len(keys), 3, dtype=np.uint32)
    b = np.full(len(keys), 2, dtype=np.uint32)
    a[0::7] = 2**22 - 2
    a[1::7] = 2**22 - 1
    a[2::7] = TOP
    b[0::14] = 1                                                   # 2^22 - 2 + 1: a new escape on output
    b[1::14] = 2**22 - 1
    b[3::7] = 2**21                                                # 2^21 + 3: no escape in either, none out
    a[4::7] = 2**21
    b[4::7] = 2**21                                                # 2^22: two plain fields make an escape
    for op in OPS:
        _check(m, tmp_path, k, [(keys, a), (keys[::2], b[::2])], op, tag=op)
    one = np.array([123456], dtype=np.uint64)
    st = _check(m, tmp_path, k, [(one, np.array([TOP], dtype=np.uint32)), (one, np.array([1], dtype=np.uint32))], "sum", tag="clamp")
    assert st["n_saturated"] == 1 and st["n_out"] == 1
    st = _check(m, tmp_path, k, [(keys, a), (keys, a), (keys, b)], "sum", tag="clamps")
    assert st["n_saturated"] == len(keys[2::7])


def _boundary_world(k):
    """input 1 holds input 0's second block's first k-mer -- a window boundary at MFX_MERGE_RANGE=1 -- in the middle of one of its blocks"""
    a = sw.random_keys(k, 2 * 4096 + 10, 21)
    rng = np.random.default_rng(22)
    b = np.setdiff1d(sw.random_keys(k, 5000, 23), a)
    b = np.union1d(b, a[[4096, 4097, 100]])
    at = int(np.searchsorted(b, a[4096]))
    assert b[at] == a[4096] and at % 4096 not in (0, 4095)
    return [(a, sw.mixed_counts(len(a), 1)), (b, rng.integers(1, 9, size=len(b)).astype(np.uint32))]


def _window_cases():
    out = []
    for k in (7, 15, 21, 31):
        for rng in (None, "1000", "1"):
            for name in ("gaps", "escapes", "nested", "boundary", "three"):
                if rng == "1" and name not in ("gaps", "boundary"):
                    continue
                if k == 7 and name == "boundary":
                    continue                                       # (4^7 k-mers: the draws above do not fit)
                out.append(pytest.param(k, name, rng, id="k%d-%s-%s" % (k, name, rng or "whole")))
    return out


@pytest.mark.parametrize("k,name,rng", _window_cases())
def test_windows(tmp_path, monkeypatch, k, name, rng):
    """a block that straddles a boundary, the writer's carry across windows, a boundary k-mer inside another input's block"""
    m = _mfx()
    if name in ("gaps", "escapes"):
        if ("kinds", k) not in _cache:
            _cache[("kinds", k)] = sw.kinds(k)
        _, keys, vals = _cache[("kinds", k)][name]
        inputs = [(keys, vals), (keys[1::3], vals[::-1][: len(keys[1::3])].copy()), (keys[:: 5], vals[::5].copy())]
    elif name == "nested":
        inputs = _world(k, "nested", (SIZES[5], SIZES[4], SIZES[1]), seed=3)
    elif name == "three":
        inputs = _world(k, "interleaved", (SIZES[4], SIZES[5], SIZES[2]), seed=4)
    else:
        inputs = _boundary_world(k)
    for name_, v in (("MFX_MERGE_RANGE", rng), ("MFX_DB_BOUNCE", "4096" if rng == "1000" else None)):
        if v is None:
            monkeypatch.delenv(name_, raising=False)
        else:
            monkeypatch.setenv(name_, v)
    nblocks = sum((len(a) + 4095) // 4096 for a, _ in inputs)
    for op in (OPS if rng != "1" else ("sum", "intersect")):
        st = _check(m, tmp_path, k, inputs, op, tag=op, load_back=(op == "sum"))
        if rng is None:
            assert st["windows"] == 1
        else:
            assert 2 <= st["windows"] <= nblocks + 1, st            # boundaries are block first k-mers


def test_filters_and_empty_results(tmp_path, monkeypatch):
    m = _mfx()
    k = 15
    monkeypatch.setenv("MFX_MERGE_RANGE", "3000")
    a, b = _world(k, "interleaved", (SIZES[5], SIZES[4]), seed=9)
    a = (a[0], np.where(np.arange(len(a[0])) % 3 == 0, 1, a[1]).astype(np.uint32))      # singletons, some of them shared with b
    for op in OPS:
        st = _check(m, tmp_path, k, [a, b], op, 1, TOP, tag=op + "_all")
        assert st["n_filtered"] == 0
        st = _check(m, tmp_path, k, [a, b], op, 2, TOP, tag=op + "_min2")
        assert st["n_filtered"] > 0
        _check(m, tmp_path, k, [a, b], op, 2, 40, tag=op + "_band")
    # everything dropped: the file mfx_db_write_flat writes for no k-mers, and no spool
    st = _check(m, tmp_path, k, [a], "sum", 0, 0, tag="none")
    assert st["n_out"] == 0 and st["n_filtered"] == len(a[0])
    assert m.db_probe(str(tmp_path / "none_out.mfxk"))["n_kmers"] == 0
    # intersect of disjoint inputs: nothing, and nothing filtered
    d = _world(k, "disjoint", (SIZES[4], SIZES[3]), seed=9)
    st = _check(m, tmp_path, k, d, "intersect", tag="disjoint")
    assert st["n_out"] == 0 and st["n_filtered"] == 0
    # one input, no filter: the input's own bytes
    src = _write(m, tmp_path / "own.mfxk", k, *a)
    for op in OPS:
        out = str(tmp_path / ("own_%s.mfxk" % op))
        st = m.db_merge([src], out, op=op)
        assert _bytes(out) == _bytes(src) and st["n_out"] == st["n_in"] == len(a[0])


def test_failure_leaves_nothing(tmp_path):
    m = _mfx()
    k = 15
    inputs = _world(k, "interleaved", (SIZES[4], SIZES[3]), seed=5)
    paths = [_write(m, tmp_path / ("f%d.mfxk" % i), k, *x) for i, x in enumerate(inputs)]
    before = [_bytes(p) for p in paths]
    out = str(tmp_path / "no_such_dir" / "out.mfxk")
    with pytest.raises(m.MfxError) as e:
        m.db_merge(paths, out)
    assert e.value.code == -6 and "cannot create the spool" in str(e.value), str(e.value)      # MFX_E_IO
    assert not os.path.exists(out) and not os.path.exists(out + ".blocks")
    assert [_bytes(p) for p in paths] == before
    # a damaged input -- a count field of a block zeroed -- ends in MFX_E_FORMAT, nothing written
    data = bytearray(before[0])
    n, nesc, nblocks, d = sw.directory(bytes(data))
    first, off, kb, vb = d[0]
    vw = off + ((4096 - 1) * kb + 63) // 64 * 8
    word = int.from_bytes(data[vw:vw + 8], "little") & ~((1 << vb) - 1)      # the first record's count field
    data[vw:vw + 8] = word.to_bytes(8, "little")
    bad = str(tmp_path / "damaged.mfxk")
    with open(bad, "wb") as f:
        f.write(bytes(data))
    out = str(tmp_path / "from_damaged.mfxk")
    with pytest.raises(m.MfxError) as e:
        m.db_merge([bad, paths[1]], out)
    assert e.value.code == -7 and "damaged.mfxk" in str(e.value) and "a count of zero" in str(e.value), str(e.value)
    assert not os.path.exists(out) and not os.path.exists(out + ".blocks")
