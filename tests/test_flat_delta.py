"""The delta-coded flat database form (mfx_db.cpp FLAT_DELTA) as a FILE FORMAT: what mfx_db_write_flat writes for sorted
k-mers is decoded here by an independent reader (numpy / Python ints, from the format's description in the header of
mfx_db.cpp) and must give back the arrays.  The GPU side of the format -- the kernel that decodes and inserts the blocks --
is pinned by tests/test_gpu_db.py against the other forms of the same database."""
import numpy as np
import pytest

from tests.delta_blocks import decode_delta, read_flat   # (the decoder lives with its inverse now)


@pytest.mark.parametrize("k,n,seed", [(21, 1, 1), (21, 4096, 2), (21, 4097, 3), (15, 20000, 4), (31, 3 * 4096 + 77, 5), (4, 200, 6)])
def test_written_blocks_decode_to_the_arrays(tmp_path, k, n, seed):
    import merfin_amd as m
    rng = np.random.default_rng(seed)
    space = 1 << (2 * k)
    keys = np.unique(rng.integers(0, space, size=min(n * 2, space), dtype=np.uint64))[:n]
    n = len(keys)
    vals = rng.integers(0, 70, size=n).astype(np.uint32)
    vals[::97] = rng.integers(2**20, 2**32 - 1, size=len(vals[::97]), dtype=np.uint64).astype(np.uint32)
    if n > 4096:
        vals[4096:4200] = 2**32 - 1                                  # a stretch of the largest count
        keys[100:200] = keys[100] + np.arange(100, dtype=np.uint64)  # consecutive k-mers
        keys = np.unique(keys)
        n = len(keys)
        vals = vals[:n]
    path = str(tmp_path / "d.mfxk")
    m.db_write_flat(path, k, keys, vals)
    kk, dk, dv = decode_delta(path)
    assert kk == k and dk == keys.tolist() and dv == vals.tolist()
    assert m.db_probe(path) == {"k": k, "format": "flat", "n_kmers": n}


def test_unsorted_k_mers_are_written_in_another_form(tmp_path, monkeypatch):
    """the delta form needs strictly ascending k-mers; anything else is written as packed (k <= 21) or plain records, and
    MFX_FLAT_DELTA=0 switches the form off"""
    import merfin_amd as m
    keys = np.array([5, 3, 9, 9], dtype=np.uint64)
    vals = np.array([1, 2, 3, 4], dtype=np.uint32)
    p = str(tmp_path / "u.mfxk")
    m.db_write_flat(p, 21, keys, vals)
    assert read_flat(p)[2] & 6 == 2
    m.db_write_flat(p, 31, keys, vals)
    assert read_flat(p)[2] & 6 == 0
    s = np.sort(np.unique(keys))
    m.db_write_flat(p, 21, s, vals[:len(s)])
    assert read_flat(p)[2] & 6 == 4
    monkeypatch.setenv("MFX_FLAT_DELTA", "0")
    m.db_write_flat(p, 21, s, vals[:len(s)])
    assert read_flat(p)[2] & 6 == 2
