"""The host side of mfx_db_merge that no device enters: the window planner (csrc/mfx_merge.h, through mfx_db_merge_plan) on hand-made
directories, and the refusals of mfx_db_merge itself on files written by db_write_flat -- each made before a device is touched, so they
hold on a machine without one."""
import os

import numpy as np
import pytest

BLOCK = 4096


def _mfx():
    import merfin_amd as m
    return m


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _firsts(nblocks, lo, step):
    return _u64([lo + i * step for i in range(nblocks)])


def _check_plan(firsts, counts, k, R):
    """the properties every plan has; returns it"""
    m = _mfx()
    plan = m.db_merge_plan(firsts, counts, k, R)
    end = 4 ** k
    cands = set(int(x) for f in firsts for x in f)
    assert plan[0][0] == 0 and plan[-1][1] == end                  # the windows cover the key space ...
    for (lo, hi, pairs, blocks), nxt in zip(plan, plan[1:] + [None]):
        assert lo < hi                                             # ... ascending and half-open ...
        if nxt is not None:
            assert nxt[0] == hi and hi in cands                    # ... each boundary a block's first k-mer
        total = 0
        for f, n, (b0, b1) in zip(firsts, counts, blocks):
            nb = (n + BLOCK - 1) // BLOCK
            assert 0 <= b0 <= b1 <= nb
            total += min(n, b1 * BLOCK) - b0 * BLOCK if b1 > b0 else 0
            # a block outside [b0, b1) holds no k-mer of [lo, hi): it ends at or below lo, or starts at or above hi
            for b in range(nb):
                b_lo, b_hi = int(f[b]), (int(f[b + 1]) if b + 1 < nb else end)
                if not (b0 <= b < b1):
                    assert b_hi <= lo or b_lo >= hi, (lo, hi, b, b_lo, b_hi)
        assert total == pairs
        if pairs > max(R, 1):                                      # above R only where no boundary allows less: one block an input at the most
            assert all(b1 - b0 <= 1 for b0, b1 in blocks), (lo, hi, pairs, blocks)
    for i, (f, n) in enumerate(zip(firsts, counts)):               # every block of every input lies in a window
        nb = (n + BLOCK - 1) // BLOCK
        seen = set()
        for _, _, _, blocks in plan:
            seen.update(range(blocks[i][0], blocks[i][1]))
        assert seen == set(range(nb)), (i, sorted(set(range(nb)) - seen))
    return plan


def test_one_window_when_everything_fits():
    firsts = [_firsts(3, 5, 1000), _firsts(2, 0, 1500)]
    counts = [3 * BLOCK, BLOCK + 5]
    plan = _check_plan(firsts, counts, 7, 1 << 26)
    assert plan == [(0, 4 ** 7, 4 * BLOCK + 5, [(0, 3), (0, 2)])]


def test_range_of_one_cuts_at_every_block_first_kmer():
    firsts = [_firsts(3, 5, 1000), _firsts(2, 0, 1500), _firsts(4, 77, 800)]
    counts = [3 * BLOCK, BLOCK + 5, 3 * BLOCK + 1]
    plan = _check_plan(firsts, counts, 11, 1)
    cands = sorted(set(int(x) for f in firsts for x in f) - {0})
    assert [w[1] for w in plan[:-1]] == cands                      # one boundary per block first k-mer (0 starts the first window)
    assert plan[0][3] == [(0, 0), (0, 1), (0, 0)]                  # below 5 only the second input has a block


def test_coinciding_first_kmers():
    f = _firsts(4, 100, 100)
    plan = _check_plan([f, f.copy(), f.copy()], [4 * BLOCK] * 3, 9, 1)
    assert [w[1] for w in plan[:-1]] == [100, 200, 300, 400]       # each boundary once
    assert plan[0][2] == 0 and plan[2][:2] == (200, 300) and plan[2][3] == [(1, 2)] * 3 and plan[2][2] == 3 * BLOCK
    plan = _check_plan([f, f.copy()], [4 * BLOCK, 3 * BLOCK + 9], 9, 2 * BLOCK)
    assert all(w[2] <= 2 * BLOCK for w in plan)


def test_an_input_without_kmers():
    f = _firsts(3, 10, 50)
    plan = _check_plan([_u64([]), f, _u64([])], [0, 2 * BLOCK + 1, 0], 8, BLOCK)
    assert all(w[3][0] == (0, 0) and w[3][2] == (0, 0) for w in plan)
    plan = _check_plan([_u64([])], [0], 8, 1)
    assert plan == [(0, 4 ** 8, 0, [(0, 0)])]


def test_one_input_far_longer_than_the_others():
    rng = np.random.default_rng(3)
    long = np.sort(rng.choice(4 ** 12, size=500, replace=False)).astype(np.uint64)
    short = _u64([7, 4 ** 12 - 5])
    for R in (1, BLOCK, 10 * BLOCK, 37 * BLOCK + 11, 1 << 26):
        plan = _check_plan([long, short, _u64([long[250]])], [500 * BLOCK - 3, BLOCK + 1, 17], 12, R)
        if R >= 10 * BLOCK:
            assert all(w[2] <= R for w in plan)
        assert len(plan) >= (500 * BLOCK) // max(R, BLOCK) // 2


def test_random_directories():
    rng = np.random.default_rng(11)
    for trial in range(30):
        k = int(rng.integers(6, 32))
        n_in = int(rng.integers(1, 7))
        firsts, counts = [], []
        for _ in range(n_in):
            nb = int(rng.integers(0, 12))
            f = np.unique(rng.integers(0, 4 ** k, size=nb, dtype=np.uint64))
            firsts.append(f)
            counts.append(0 if len(f) == 0 else (len(f) - 1) * BLOCK + int(rng.integers(1, BLOCK + 1)))
        _check_plan(firsts, counts, k, int(rng.choice([1, 5000, 3 * BLOCK, 1 << 26])))


# ---- the refusals of mfx_db_merge: MFX_E_INVAL (-1) or MFX_E_FORMAT (-7), the file named, nothing written
def _flat(m, path, k, n=100, seed=0):
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, min(4 ** k, 1 << 24), size=n, dtype=np.uint64))
    m.db_write_flat(str(path), k, keys, np.ones(len(keys), dtype=np.uint32))
    return str(path)


def _refused(m, tmp_path, paths, code, *texts, **kw):
    out = str(tmp_path / "out.mfxk")
    with pytest.raises(m.MfxError) as e:
        m.db_merge(paths, kw.pop("out", out), **kw)
    assert e.value.code == code, str(e.value)
    for t in texts:
        assert t in str(e.value), str(e.value)
    assert "hip" not in str(e.value).lower()                       # refused before a device is asked for
    assert not os.path.exists(out) and not os.path.exists(out + ".blocks")


def test_refusals_need_no_device(tmp_path, monkeypatch):
    m = _mfx()
    a = _flat(m, tmp_path / "a.mfxk", 15)
    b = _flat(m, tmp_path / "b.mfxk", 15, seed=1)
    _refused(m, tmp_path, [a, _flat(m, tmp_path / "k17.mfxk", 17)], -1, "k17.mfxk", "17-mers", "15-mers")
    placed = str(tmp_path / "placed.mfxk")
    m.db_write_flat(str(tmp_path / "canon.mfxk"), 15, np.arange(50, dtype=np.uint64), np.ones(50, dtype=np.uint32))
    m.db_convert_placed(str(tmp_path / "canon.mfxk"), placed)
    _refused(m, tmp_path, [a, placed], -7, "placed.mfxk", "placed database")
    monkeypatch.setenv("MFX_FLAT_DELTA", "0")
    packed = _flat(m, tmp_path / "packed.mfxk", 15, seed=2)
    monkeypatch.setenv("MFX_FLAT_PACKED", "0")
    plain = _flat(m, tmp_path / "plain.mfxk", 15, seed=3)
    monkeypatch.delenv("MFX_FLAT_DELTA")
    monkeypatch.delenv("MFX_FLAT_PACKED")
    _refused(m, tmp_path, [packed, a], -7, "packed.mfxk", "packed flat file", "run `merfin -convert` first")
    _refused(m, tmp_path, [a, plain], -7, "plain.mfxk", "plain flat file", "run `merfin -convert` first")
    text = tmp_path / "print.txt"
    text.write_text("AAAAAAAAAAAAAAC\t3\nAAAAAAAAAAAAAAG\t1\n")
    _refused(m, tmp_path, [str(text), a], -7, "print.txt", "run `merfin -convert` first")
    (tmp_path / "db.meryl").mkdir()
    _refused(m, tmp_path, [a, str(tmp_path / "db.meryl")], -7, "db.meryl", "meryl directory", "run `merfin -convert` first")
    _refused(m, tmp_path, [a, str(tmp_path / "absent.mfxk")], -6, "absent.mfxk")
    before = open(a, "rb").read()
    _refused(m, tmp_path, [a, b], -1, "is the input", "b.mfxk", out=b)
    os.link(a, str(tmp_path / "alias.mfxk"))                       # the same file under another name: compared by device and inode
    _refused(m, tmp_path, [a, b], -1, "is the input", "a.mfxk", out=str(tmp_path / "alias.mfxk"))
    assert open(a, "rb").read() == before
    _refused(m, tmp_path, [], -1, "0 inputs")
    _refused(m, tmp_path, [a] * 65, -1, "65 inputs")
    _refused(m, tmp_path, [a, b], -1, "unknown operation 7", op=7)
    _refused(m, tmp_path, [a, b], -1, "min 5 > max 4", min_count=5, max_count=4)
    with pytest.raises(KeyError):
        m.db_merge([a, b], str(tmp_path / "out.mfxk"), op="difference")
    # a damaged input: the header claims more k-mers than the directory holds
    data = bytearray(before)
    data[16:24] = (10 ** 6).to_bytes(8, "little")
    (tmp_path / "damaged.mfxk").write_bytes(bytes(data))
    _refused(m, tmp_path, [a, str(tmp_path / "damaged.mfxk")], -7, "damaged.mfxk")
