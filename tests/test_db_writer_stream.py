"""The streamed database writer on the host (mfx_db_writer_open_streamed + mfx_db_writer_append_sorted): spool, carry and close without a
device.  Every file is compared byte for byte with what mfx_db_write_flat -- the plain writer, not the code under test -- makes of the
same arrays; no tolerance anywhere."""
import os

import numpy as np
import pytest

from tests import stream_worlds as sw

BLOCK = sw.BLOCK


def _m():
    import merfin_amd as m
    return m


def _plain(tmp_path, k, keys, vals):
    """the bytes of the plain writer's file"""
    p = str(tmp_path / "plain.mfxk")
    _m().db_write_flat(p, k, keys, vals)
    with open(p, "rb") as f:
        return f.read()


def _pieces(n, size):
    return [(o, min(n, o + size)) for o in range(0, n, size)] if n else [(0, 0)]


def _stream(tmp_path, k, keys, vals, size, name="s.mfxk", check=None):
    """the arrays through a streamed writer in appends of `size` k-mers; the file's bytes"""
    m = _m()
    p = str(tmp_path / name)
    if os.path.exists(p):
        os.remove(p)
    w = m.DbWriter(p, k, streamed=True)
    assert os.path.exists(p + ".blocks") and not os.path.exists(p)
    for lo, hi in _pieces(len(keys), size):
        assert w.append_sorted(keys[lo:hi], vals[lo:hi]) == hi - lo
    assert os.path.exists(p + ".blocks") and not os.path.exists(p)           # nothing at path, a spool present, before close
    info = w.info()
    assert w.close() == len(keys)
    assert not os.path.exists(p + ".blocks")
    with open(p, "rb") as f:
        data = f.read()
    if check is not None:
        check(info, data)
    return data


def _info_agrees(k, keys, vals):
    n = len(keys)

    def check(info, data):
        assert info["kmers"] == n and info["blocks"] == n // BLOCK
        if n == 0:
            assert info == {"kmers": 0, "blocks": 0, "escapes": 0, "spool_bytes": 0, "held_bytes": 0}
            return
        fn, fesc, nblocks, d = sw.directory(data)
        assert fn == n and nblocks == (n + BLOCK - 1) // BLOCK
        table = sw.HEADER + 8 + 16 * (nblocks + 1)
        carry = n % BLOCK
        if carry == 0:                                                        # every block is in the spool: the file is the spool and what frames it
            assert info["spool_bytes"] == len(data) - sw.HEADER - 8 - 16 * (nblocks + 1) - 12 * fesc
            assert info["escapes"] == fesc
        else:                                                                 # ... all but the last, partial block, which close codes
            assert info["spool_bytes"] == d[nblocks - 1][1] - table
            vb = d[nblocks - 1][3]
            assert info["escapes"] == fesc - int((vals[n - carry:] >= (1 << vb) - 1).sum())
        assert d[nblocks][1] == len(data) - 12 * fesc and d[0][1] == table
        assert info["held_bytes"] == 16 * info["blocks"] + 12 * info["escapes"] + 12 * carry
    return check


@pytest.mark.parametrize("k", [7, 21, 31])
@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 3 * 4096])
def test_sizes_and_splits(tmp_path, k, n):
    k, keys, vals = sw.sized(k, n)
    want = _plain(tmp_path, k, keys, vals)
    for size in (1, 4095, 4096, 4097, max(n, 1)):
        got = _stream(tmp_path, k, keys, vals, size, check=_info_agrees(k, keys, vals))
        assert got == want, (k, n, size)


def _kind_worlds():
    out = []
    for k in (7, 21, 31):
        for name, world in sw.kinds(k).items():
            out.append(pytest.param(world, id="%s-k%d" % (name, k)))
    out.append(pytest.param(sw.all_7mers(), id="all7mers"))
    out.append(pytest.param(sw.pair62(), id="pair62"))
    return out


@pytest.mark.parametrize("world", _kind_worlds())
def test_kinds_of_block(tmp_path, world):
    k, keys, vals = world
    want = _plain(tmp_path, k, keys, vals)
    for size in (len(keys), 4097, 1000):
        assert _stream(tmp_path, k, keys, vals, size, check=_info_agrees(k, keys, vals)) == want, size


def test_the_kinds_are_what_they_are_named(tmp_path):
    """the plain writer's directory shows the widths the worlds were built for: the comparison above covers those cases"""
    def first(world):
        k, keys, vals = world
        n, nesc, nblocks, d = sw.directory(_plain(tmp_path, k, keys, vals))
        return nesc, nblocks, d
    nesc, nblocks, d = first(sw.all_7mers())
    assert nblocks == 4 and all(e[2] == 1 for e in d[:4])
    nesc, nblocks, d = first(sw.pair62())
    assert nblocks == 1 and d[0][2] == 62 and nesc == 1
    kinds = sw.kinds(21)
    nesc, nblocks, d = first(kinds["vb2"])
    assert nesc == 0 and all(e[3] == 2 for e in d[:nblocks])
    nesc, nblocks, d = first(kinds["vb22"])
    assert nesc == 0 and d[0][3] == 22 and d[nblocks - 1][3] == 22
    nesc, nblocks, d = first(kinds["escapes"])
    assert nesc == int((kinds["escapes"][2] >= 2**22 - 1).sum()) > 1000
    nesc, nblocks, d = first(kinds["escape_cheaper"])
    assert nesc == 6 and d[0][3] == 2
    nesc, nblocks, d = first(kinds["widen_cheaper"])
    assert nesc == 0 and d[0][3] == 20
    nesc, nblocks, d = first(kinds["tie"])
    assert nesc == 128 and d[0][3] == 2                                       # 4096 x 2 + 96 x 128 == 4096 x 5: the smaller width
    widths = [e[2] for kk in (7, 21, 31) for e in first(sw.kinds(kk)["gaps"])[2][:2]]
    assert any(64 % kb for kb in widths), widths                              # differences that straddle words


@pytest.mark.parametrize("streamed", [True, False])
def test_refused_appends_add_nothing(tmp_path, streamed):
    m = _m()
    k, keys, vals = sw.sized(21, 3 * BLOCK + 500, seed=9)
    want = _plain(tmp_path, k, keys, vals)
    p = str(tmp_path / "r.mfxk")
    w = m.DbWriter(p, k, streamed=streamed)
    a, b = BLOCK + 100, 3 * BLOCK + 7
    w.append_sorted(keys[:a], vals[:a])
    before = w.info()

    def refused(kk, vv, text):
        with pytest.raises(m.MfxError) as e:
            w.append_sorted(kk, vv)
        assert e.value.code == -1 and text in str(e.value), str(e.value)
        assert w.info() == before
        if streamed:
            assert os.path.getsize(p + ".blocks") == before["spool_bytes"]

    refused(keys[:a], vals[:a], "not above the writer's last k-mer %d" % int(keys[a - 1]))         # too low
    refused(keys[a - 1:b], vals[a - 1:b], "not above the writer's last k-mer %d" % int(keys[a - 1]))   # its first k-mer is the last one held
    bad = keys[a:b].copy()
    bad[BLOCK + 50] = bad[BLOCK + 49]                                                              # a repeat deep inside, beyond a block
    refused(bad, vals[a:b], "not strictly ascending")
    bad = keys[a:b].copy()
    bad[3], bad[4] = bad[4], bad[3]
    refused(bad, vals[a:b], "not strictly ascending")
    w.append_sorted(keys[a:b], vals[a:b])
    w.append_sorted(keys[:0], vals[:0])                                                            # an append of nothing
    w.append_sorted(keys[b:], vals[b:])
    assert w.info()["kmers"] == len(keys)
    if not streamed:
        assert w.info()["held_bytes"] == 12 * len(keys) and w.info()["spool_bytes"] == 0
    assert w.close() == len(keys)
    with open(p, "rb") as f:
        assert f.read() == want
    assert not os.path.exists(p + ".blocks")


def test_abort_open_failure_and_nothing(tmp_path):
    m = _m()
    k, keys, vals = sw.sized(21, BLOCK + 9)
    p = str(tmp_path / "a.mfxk")
    w = m.DbWriter(p, k, streamed=True)
    w.append_sorted(keys, vals)
    assert os.path.getsize(p + ".blocks") == w.info()["spool_bytes"] > 0
    w.abort()
    assert not os.path.exists(p) and not os.path.exists(p + ".blocks")
    w = m.DbWriter(p, k, streamed=True)                                       # dropped without close: as abort
    w.append_sorted(keys, vals)
    del w
    assert not os.path.exists(p) and not os.path.exists(p + ".blocks")
    with pytest.raises(m.MfxError) as e:                                      # a spool that cannot be created
        m.DbWriter(str(tmp_path / "no" / "such" / "dir.mfxk"), k, streamed=True)
    assert e.value.code == -6 and "cannot create the spool" in str(e.value)
    with pytest.raises(m.MfxError) as e:
        m.DbWriter(p, 32, streamed=True)
    assert e.value.code == -1 and not os.path.exists(p + ".blocks")
    # a close of nothing: the plain writer's file of nothing
    for kk in (21, 31):
        assert _stream(tmp_path, kk, keys[:0], vals[:0], 1) == _plain(tmp_path, kk, keys[:0], vals[:0])
