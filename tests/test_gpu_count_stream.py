"""The streamed database writer through tables on the device (mfx_index_write_db_streamed, DbWriter(streamed=True).append): the encoder
kernels of csrc/mfx_sort.hip, the carry across key ranges and appends, the roll-back of a refused append.  Every file is compared byte for
byte with mfx_db_write_flat -- the host writer -- of the same arrays, and loaded back through the decode kernel."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import stream_worlds as sw, synth_reads as sr

pytestmark = pytest.mark.gpu

_cache = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _kinds(k):
    if k not in _cache:
        _cache[k] = sw.kinds(k)
        if k == 31:
            _cache[k]["pair62"] = sw.pair62()
        if k == 7:
            _cache[k] = {"all7mers": sw.all_7mers(), "gaps": _cache[k]["gaps"]}
    return _cache[k]


def _plain(m, tmp_path, k, keys, vals):
    p = str(tmp_path / "plain.mfxk")
    m.db_write_flat(p, k, keys, vals)
    with open(p, "rb") as f:
        return f.read()


def _table(m, k, keys, vals, side):
    ix = m.Index(k, len(keys) + 64)
    (ix.add_asm if side else ix.add_read)(keys, vals)
    return ix


def _same_table(ix, keys, vals, side):
    ek, er, ea = ix.export()
    np.testing.assert_array_equal(ek, keys)
    np.testing.assert_array_equal(ea if side else er, vals)
    assert not (er if side else ea).any()


def _set_range(monkeypatch, rng, bounce):
    for name, v in (("MFX_WRITE_DB_RANGE", rng), ("MFX_DB_BOUNCE", bounce)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


# MFX_WRITE_DB_RANGE=1: one key range per bin of the top 12 key bits -- thousands of ranges below one block, the carry growing over them;
# kept to two worlds a k.  1000: the carry crosses every range, and the packed bytes of a range take several bounce pieces of 4096 bytes.
def _cases():
    out = []
    for k in (5, 7, 15, 21, 31):
        for name in _kinds(k):
            for rng in (None, "1000", "1"):
                if rng == "1" and name not in ("gaps", "escapes", "all7mers"):
                    continue
                out.append(pytest.param(k, name, rng, id="k%d-%s-%s" % (k, name, rng or "whole")))
    return out


@pytest.mark.parametrize("k,name,rng", _cases())
def test_tables_written_streamed(tmp_path, monkeypatch, k, name, rng):
    m = _mfx()
    _, keys, vals = _kinds(k)[name]
    want = _plain(m, tmp_path, k, keys, vals)
    _set_range(monkeypatch, rng, "4096" if rng == "1000" else None)
    for side in ((0, 1) if rng != "1" else (0,)):
        ix = _table(m, k, keys, vals, side)
        out = str(tmp_path / ("s%d.mfxk" % side))
        assert ix.write_db(out, side, streamed=True) == len(keys)
        assert not os.path.exists(out + ".blocks")
        with open(out, "rb") as f:
            assert f.read() == want, (k, name, rng, side)
        _same_table(ix, keys, vals, side)                         # the table is unchanged
        assert ix.write_db(str(tmp_path / "other.mfxk"), 1 - side, streamed=True) == 0      # the other side: nothing, and no spool stays
        assert not os.path.exists(str(tmp_path / "other.mfxk.blocks"))
        back = m.Index(k, len(keys) + 64)                         # a round trip through the decode kernel
        back.load_db(out, side)
        _same_table(back, keys, vals, side)


@pytest.mark.parametrize("k", [15, 21, 31])
def test_ranged_counters_into_one_streamed_writer(tmp_path, monkeypatch, k):
    m = _mfx()
    _, reads = sr.reads_world(k, 2400 + k, sizes=(9000, 4096, 500), n_reads=600)
    rk, rv = po.count_kmers(k, reads)
    n, top = len(rk), 4 ** k
    a, b = int(rk[n // 3]), int(rk[2 * n // 3])
    want = _plain(m, tmp_path, k, rk, rv)
    one = m.Index(k, 2000)
    one.count_reads_all(reads, batch_bases=4096)
    out = str(tmp_path / "one.mfxk")
    assert one.write_db(out, streamed=True) == n
    with open(out, "rb") as f:
        assert f.read() == want
    parts = []
    for lo, hi in ((0, a), (a, b), (b, top)):
        ix = m.Index(k, 2000)
        ix.count_reads_range(reads, lo, hi, batch_bases=4096)
        parts.append(ix)
    before = [p.export() for p in parts]
    empty = m.Index(k, 2000)
    out = str(tmp_path / "passes.mfxk")
    for rng in (None, "1000"):
        _set_range(monkeypatch, rng, None)
        if os.path.exists(out):
            os.remove(out)
        w = m.DbWriter(out, k, streamed=True)
        assert w.append(empty) == 0                                # an append of an empty table, first and in the middle
        added = [w.append(parts[0]), w.append(empty), w.append(parts[1])]
        assert added == [n // 3, 0, 2 * n // 3 - n // 3]
        held = w.info()
        assert held["kmers"] == 2 * n // 3 and held["blocks"] == held["kmers"] // sw.BLOCK
        assert held["spool_bytes"] == os.path.getsize(out + ".blocks")
        assert held["held_bytes"] == 16 * held["blocks"] + 12 * held["escapes"] + 12 * (held["kmers"] % sw.BLOCK)
        for late in (parts[0], parts[1]):                          # out of order: refused, nothing added, the spool rolled back
            with pytest.raises(m.MfxError) as e:
                w.append(late)
            assert e.value.code == -1 and "not above the writer's last k-mer %d" % int(rk[2 * n // 3 - 1]) in str(e.value), str(e.value)
            assert w.info() == held and os.path.getsize(out + ".blocks") == held["spool_bytes"]
        with pytest.raises(m.MfxError) as e:
            w.append(parts[2], side=2)
        assert e.value.code == -1 and "mfx_db_writer_append_index: side 2" in str(e.value)
        assert w.append(parts[2]) == n - 2 * n // 3
        assert not os.path.exists(out) and os.path.exists(out + ".blocks")
        assert w.close() == n
        assert not os.path.exists(out + ".blocks")
        with open(out, "rb") as f:
            assert f.read() == want, rng
        assert m.db_probe(out) == {"k": k, "format": "flat", "n_kmers": n}
    for p, was in zip(parts, before):                              # the tables are unchanged
        for x, y in zip(p.export(), was):
            np.testing.assert_array_equal(x, y)


def test_host_and_device_appends_mix(tmp_path, monkeypatch):
    """append_sorted and append into one streamed writer: the carry goes from the host to the device and back"""
    m = _mfx()
    k = 21
    _, keys, vals = _kinds(k)["escapes"]
    want = _plain(m, tmp_path, k, keys, vals)
    cuts = [0, 700, 700 + sw.BLOCK + 3, 2 * sw.BLOCK - 1, len(keys)]
    _set_range(monkeypatch, "1500", "4096")
    out = str(tmp_path / "mix.mfxk")
    w = m.DbWriter(out, k, streamed=True)
    for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        if i % 2 == 0:
            assert w.append_sorted(keys[lo:hi], vals[lo:hi]) == hi - lo
        else:
            assert w.append(_table(m, k, keys[lo:hi], vals[lo:hi], 0)) == hi - lo
    with pytest.raises(m.MfxError) as e:                          # a table that starts at the last k-mer held
        w.append(_table(m, k, keys[-1:], vals[-1:], 0))
    assert e.value.code == -1 and "not above the writer's last k-mer %d" % int(keys[-1]) in str(e.value)
    assert w.close() == len(keys)
    with open(out, "rb") as f:
        assert f.read() == want
    # abort after device appends: nothing stays
    w = m.DbWriter(out + "2", k, streamed=True)
    assert w.append(_table(m, k, keys, vals, 1), side=1) == len(keys)
    w.abort()
    assert not os.path.exists(out + "2") and not os.path.exists(out + "2.blocks")
