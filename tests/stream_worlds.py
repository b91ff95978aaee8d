"""Sorted k-mer databases for the tests of the streamed database writer (tests/test_db_writer_stream.py on the host,
tests/test_gpu_count_stream.py through tables on the device): every kind of delta-coded block the block rule (csrc/mfx_delta.h) tells
apart, a few blocks each.  Every world is (k, k-mers ascending, counts); counts are never zero, so a table that took them on one side
gives them back."""
import numpy as np

BLOCK = 4096
HEADER = 32                                                        # FlatHeader (csrc/mfx_db.cpp): magic, k, flags, n, n_escape


def random_keys(k, n, seed):
    """n distinct k-mers in ascending order, gaps of every width up to the whole space"""
    rng = np.random.default_rng(seed)
    space = 1 << (2 * k)
    if n >= space:
        return np.arange(space, dtype=np.uint64)
    keys = np.unique(rng.integers(0, space, size=min(2 * n + 16, space), dtype=np.uint64))
    while len(keys) < n:
        keys = np.unique(np.concatenate([keys, rng.integers(0, space, size=n, dtype=np.uint64)]))
    pick = np.sort(rng.choice(len(keys), size=n, replace=False))
    return keys[pick]


def mixed_counts(n, seed):
    """mostly small counts, some of every width, a few escapes"""
    rng = np.random.default_rng(seed + 1000)
    v = rng.integers(1, 60, size=n).astype(np.uint32)
    if n:
        v[::53] = rng.integers(1, 1 << 21, size=len(v[::53])).astype(np.uint32)
        v[::401] = np.uint32(2**32 - 1)
        v[7::977] = np.uint32(2**22 - 1)
    return v


def sized(k, n, seed=0):
    return k, random_keys(k, n, 17 * k + n + seed), mixed_counts(n, k + n + seed)


def kinds(k):
    """name -> (k, k-mers, counts): the kinds of block, 1 to 4 blocks each"""
    rng = np.random.default_rng(100 + k)
    out = {}
    n = 2 * BLOCK + 1234
    keys = random_keys(k, min(n, 4 ** k), 5 + k)
    n = len(keys)
    out["gaps"] = (k, keys, mixed_counts(n, 3))                                       # fields that straddle words, every width
    out["vb2"] = (k, keys, rng.integers(1, 3, size=n).astype(np.uint32))              # counts <= 2
    v = rng.integers(1, 2**22 - 1, size=n).astype(np.uint32)
    v[0] = v[-1] = np.uint32(2**22 - 2)
    out["vb22"] = (k, keys, v)                                                        # counts up to 2^22 - 2: none escapes
    v = rng.integers(1, 9, size=n).astype(np.uint32)
    v[::5] = np.uint32(2**22 - 1)
    v[1::7] = np.uint32(2**32 - 1)
    out["escapes"] = (k, keys, v)
    b = min(BLOCK, n)
    v = np.ones(n, dtype=np.uint32)
    v[rng.choice(b, size=min(6, b), replace=False)] = 10**6
    out["escape_cheaper"] = (k, keys, v)                                              # 4090 ones and 6 counts of 10^6: 6 escapes
    v = np.ones(n, dtype=np.uint32)
    v[:b][rng.permutation(b)[:b // 2]] = 10**6
    out["widen_cheaper"] = (k, keys, v)                                               # half and half: 20 bits for every count
    # a cost tie in the first block: 4096 x 2 + 96 x 128 = 4096 x 5 -- the smaller width, 2 bits and 128 escapes, wins
    v = rng.integers(1, 3, size=n).astype(np.uint32)
    if b == BLOCK:
        v[:b][rng.permutation(b)[:128]] = 20
    out["tie"] = (k, keys, v)
    return out


def all_7mers():
    """every 7-mer: each difference is 1 (kb = 1), four exact blocks"""
    return 7, np.arange(4 ** 7, dtype=np.uint64), mixed_counts(4 ** 7, 7)


def pair62():
    """k = 31, the smallest and the largest k-mer: one difference of 62 bits"""
    return 31, np.array([0, 2**62 - 1], dtype=np.uint64), np.array([3, 2**32 - 1], dtype=np.uint32)


def directory(data):
    """(n, n_escape, nblocks, [(first k-mer, offset, kb, vb)] with the closing entry) of a delta-coded flat file's bytes"""
    assert data[:8] == b"MFXKMER1"
    flags = int(np.frombuffer(data, dtype="<u4", count=1, offset=12)[0])
    n, nesc = (int(x) for x in np.frombuffer(data, dtype="<u8", count=2, offset=16))
    assert flags & 4, "not delta-coded"
    nblocks = int(np.frombuffer(data, dtype="<u8", count=1, offset=HEADER)[0])
    d = np.frombuffer(data, dtype="<u8", count=2 * (nblocks + 1), offset=HEADER + 8).reshape(-1, 2)
    return n, nesc, nblocks, [(int(a), int(b) & (2**48 - 1), (int(b) >> 48) & 0xff, int(b) >> 56) for a, b in d]
