"""What of the sorted join (mfx_db_join_*, csrc/mfx_join.h, `merfin -join`) needs no device: the refusals of the two API calls, each by
message and with the outputs untouched; the refusals of the CLI flag (cli/args.h: check_join_flags); and the kernel's tile cuts, lane
shares and ownership rule as mfx_db_join_host runs them on the host -- the text the kernel's lanes run -- against a numpy join, with an
equal pair on every lane and tile boundary."""
import os
import subprocess

import numpy as np
import pytest

from tests import stream_worlds as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "merfin_amd", "bin", "merfin")


def _mfx():
    import merfin_amd as m
    return m


def _write(m, path, k, n, seed):
    keys = sw.random_keys(k, n, seed)
    m.db_write_flat(str(path), k, keys, sw.mixed_counts(len(keys), seed))
    return str(path)


# ---- the API: refused before a device is touched (this machine has none: a call that went on would end in a HIP error)

def _refused(m, read, asm, code, text):
    for call in (lambda: m.db_join_completeness(read, asm, 20.0), lambda: m.db_join_spectrum(read, asm, copies=4, max_mult=100)):
        with pytest.raises(m.MfxError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert "hip" not in str(e.value).lower()


def test_api_refusals(tmp_path, monkeypatch):
    m = _mfx()
    a = _write(m, tmp_path / "a.mfxk", 21, 4097, 1)
    b = _write(m, tmp_path / "b.mfxk", 21, 500, 2)
    k15 = _write(m, tmp_path / "k15.mfxk", 15, 500, 3)
    _refused(m, a, k15, -1, "holds 15-mers, '%s' 21-mers: the inputs are of one k" % a)
    _refused(m, k15, b, -1, "the inputs are of one k")
    # k > 31: mfx_db_write_flat takes the k-mers' low words; the file says k = 32
    k32 = str(tmp_path / "k32.mfxk")
    m.db_write_flat(k32, 32, np.array([1, 5, 9], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint32))
    _refused(m, k32, b, -1, "'%s' holds 32-mers: the sorted join takes k <= 31" % k32)
    _refused(m, a, k32, -1, "holds 32-mers: the sorted join takes k <= 31")
    # a placed file
    placed = str(tmp_path / "placed.mfxk")
    x, rc = sw.random_keys(21, 500, 9), np.zeros(500, dtype=np.uint64)
    fwd = x.copy()
    for _ in range(21):                                            # a placed database holds canonical k-mers
        rc = (rc << np.uint64(2)) | ((x & np.uint64(3)) ^ np.uint64(2))
        x = x >> np.uint64(2)
    canon = np.unique(np.minimum(fwd, rc))
    m.db_write_flat(str(tmp_path / "canon.mfxk"), 21, canon, np.ones(len(canon), dtype=np.uint32))
    m.db_convert_placed(str(tmp_path / "canon.mfxk"), placed)
    _refused(m, a, placed, -7, "'%s' is a placed database; the inputs are sorted by k-mer" % placed)
    _refused(m, placed, a, -7, "is a placed database")
    # the wrong forms: packed and plain flat files, text, a meryl-like directory, nothing
    monkeypatch.setenv("MFX_FLAT_DELTA", "0")
    packed = _write(m, tmp_path / "packed.mfxk", 21, 300, 4)
    monkeypatch.delenv("MFX_FLAT_DELTA")
    _refused(m, packed, a, -7, "'%s' is a packed flat file, not a sorted one: run `merfin -convert` first" % packed)
    plain = str(tmp_path / "plain.mfxk")
    m.db_write_flat(plain, 21, np.array([9, 5, 1], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint32))      # (not ascending: no sorted form)
    _refused(m, a, plain, -7, "flat file, not a sorted one: run `merfin -convert` first")
    text = tmp_path / "print.txt"
    text.write_text("ACGTACGTACGTACGTACGTA\t3\n")
    _refused(m, a, str(text), -7, "is not a flat k-mer file (`meryl print` text?); the inputs are sorted flat databases: run `merfin -convert` first")
    (tmp_path / "db.meryl").mkdir()
    _refused(m, str(tmp_path / "db.meryl"), a, -7, "is a meryl directory; the inputs are sorted flat databases: run `merfin -convert` first")
    _refused(m, a, str(tmp_path / "absent.mfxk"), -6, "does not exist")


def test_api_bounds_and_nulls(tmp_path):
    import ctypes as C
    m = _mfx()
    L = m.load_library()
    a = _write(m, tmp_path / "a.mfxk", 21, 100, 1)
    for copies, max_mult, text in ((0, 100, "copies = 0 is outside [1, 6]"), (7, 100, "copies = 7 is outside [1, 6]"), (4, 3, "max_mult = 3 is outside [4, 65536]"),
                                   (4, 65537, "max_mult = 65537 is outside [4, 65536]")):
        with pytest.raises(m.MfxError) as e:
            m.db_join_spectrum(a, a, copies=copies, max_mult=max_mult)
        assert e.value.code == -1 and text in str(e.value), str(e.value)
    from merfin_amd.binding import DbJoinOpts
    o = DbJoinOpts(0, 0, 2**32 - 1, 20.0, 0, None, None, 4, 100)
    t = (C.c_double * 64)()
    n = C.c_uint64(0)
    img = (C.c_uint64 * (6 * 101))()
    assert L.mfx_db_join_completeness(a.encode(), a.encode(), C.byref(o), t, None, None) == -1 and b"null argument" in L.mfx_last_error()
    assert L.mfx_db_join_completeness(a.encode(), a.encode(), None, t, t, None) == -1
    assert L.mfx_db_join_completeness(None, a.encode(), C.byref(o), t, t, None) == -1
    assert L.mfx_db_join_spectrum(a.encode(), a.encode(), C.byref(o), None, C.byref(n), None) == -1 and b"null argument" in L.mfx_last_error()
    assert L.mfx_db_join_spectrum(a.encode(), a.encode(), C.byref(o), img, None, None) == -1
    o.n_prob = 3                                                   # a -prob table announced and not given
    assert L.mfx_db_join_completeness(a.encode(), a.encode(), C.byref(o), t, t, None) == -1


# ---- the CLI flag

JOIN = ["-join", "-readmers", "{T}/a.mfxk", "-seqmers", "{T}/b.mfxk"]
OTHER = "-join is a way to run -completeness and -spectrum: it does not take another report type (-hist, -dump, -track, the variant modes)."

CASES = [
    (["-hist", "-sequence", "{T}/r.fa", "-output", "{T}/o", "-peak", "9"] + JOIN, [OTHER]),
    (["-dump", "-sequence", "{T}/r.fa", "-output", "{T}/o", "-peak", "9"] + JOIN, [OTHER]),
    (["-track", "-sequence", "{T}/r.fa", "-output", "{T}/o", "-peak", "9"] + JOIN, [OTHER]),
    (["-filter", "-sequence", "{T}/r.fa", "-vcf", "x.vcf", "-output", "{T}/o"] + JOIN, [OTHER]),
    (["-completeness", "-peak", "9", "-join", "-seqmers", "{T}/b.mfxk", "-reads", "{T}/r.fa", "-k", "21"],
     ["-join joins two databases: it does not take -reads (count them first: -count)."]),
    (["-completeness", "-peak", "9", "-join", "-readmers", "{T}/a.mfxk", "-sequence", "{T}/r.fa"],
     ["-join joins two databases: it takes the assembly as -seqmers, not as -sequence (merfin -count -reads asm.fasta -k K -output asm.mfxk)."]),
    (["-completeness", "-peak", "9"] + JOIN + ["-devices", "0-1", "-sharded"],
     ["-join does not take -sharded: the windows it joins live on one device, and no table is built.", "-join runs on one device (-device d, or -devices naming one)."]),
    (["-completeness", "-peak", "9"] + JOIN + ["-devices", "0,1"], ["-join runs on one device (-device d, or -devices naming one)."]),
    (["-completeness", "-peak", "9"] + JOIN + ["-index", "{T}/i.idx"], ["-join does not take -index: it builds no table."]),
    (["-spectrum", "-output", "{T}/o", "-peak", "auto"] + JOIN, ["-join does not take -peak auto: the peak is read off a table; give -peak <number>."]),
    (["-spectrum", "-output", "{T}/o"] + JOIN + ["-index", "{T}/i.idx", "-peak", "auto"],
     ["-join does not take -index: it builds no table.", "-join does not take -peak auto: the peak is read off a table; give -peak <number>."]),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_cli_refusal(tmp_path, case):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    for name in ("a.mfxk", "b.mfxk", "r.fa"):
        (tmp_path / name).write_text(">r0\nACGTACGTACGTACGTACGTACGTACGT\n")      # (refused before a file is opened)
    argv, lines = CASES[case]
    r = subprocess.run([EXE] + [a.replace("{T}", str(tmp_path)) for a in argv], capture_output=True, text=True)
    assert r.returncode == 1, r.stderr
    assert r.stderr.startswith("usage: ")
    # the usage text, the entry of -join behind it (it says how an assembly's database is made), then the lines of this command line
    head, sep, tail = r.stderr.partition("  -completeness and -spectrum without a table:\n")
    assert sep, r.stderr
    entry, _, mine = tail.partition("\n\n")
    assert "-join " in entry and "merfin -count -reads asm.fasta -k K -output asm.mfxk" in entry
    assert [l for l in mine.splitlines() if l.startswith("-join ")] == lines, r.stderr
    assert "ERROR: HIP device" not in r.stderr                            # refused before a device is asked for
    assert not os.path.exists(str(tmp_path / "o.spectra-cn.hist"))


# ---- the kernel's walk on the host

def _plain(rk, rv, ak, av):
    u = np.union1d(rk, ak)
    r = np.zeros(len(u), dtype=np.uint32)
    a = np.zeros(len(u), dtype=np.uint32)
    r[np.searchsorted(u, rk)] = rv
    a[np.searchsorted(u, ak)] = av
    return u, r, a


def _walk_is_plain(m, rk, rv, ak, av):
    keys, r, a = m.db_join_host(rk, rv, ak, av)
    wk, wr, wa = _plain(rk, rv, ak, av)
    assert np.array_equal(keys, wk) and np.array_equal(r, wr) and np.array_equal(a, wa), (len(rk), len(ak), len(keys), len(wk))


def boundary_world(grain, shift, total, seed=0):
    """(read k-mers, asm k-mers) with a k-mer of both on every multiple of `grain` in merged order: position p holds its read record and p + 1 the
    asm twin when (p + shift) % grain == grain - 1 -- shift 0: the boundary falls between the twins; 1: just behind the pair; grain - 1: just in
    front of it.  The positions between alternate, three read-only and three asm-only."""
    rng = np.random.default_rng(seed)
    rk, ak = [], []
    key, p = 10, 0
    while p < total:
        if (p + shift) % grain == grain - 1:
            rk.append(key); ak.append(key); p += 2
        else:
            (rk if (p // 3) % 2 else ak).append(key); p += 1
        key += 1 + int(rng.integers(0, 3))
    return np.array(rk, dtype=np.uint64), np.array(ak, dtype=np.uint64)


def test_usage_without_join_is_unchanged():
    """a command line that does not name -join gets the usage text as it was"""
    r = subprocess.run([EXE, "-bogus"], capture_output=True, text=True)
    assert r.returncode == 1 and "-join" not in r.stderr


def test_grain_constants():
    per, tile = _mfx().db_join_grain()
    assert tile % per == 0 and tile // per == 256 and per >= 2     # a tile is 256 lane shares: a pair on every lane boundary is one on every tile boundary


@pytest.mark.parametrize("sizes", [(0, 0), (1, 0), (0, 1), (1, 1), (7, 9), (2047, 1), (2048, 2048), (4095, 4097), (3 * 4096 + 17, 4096), (5, 3 * 4096 + 17)])
def test_host_walk_random(sizes):
    m = _mfx()
    nr, na = sizes
    for seed, space in ((1, 2 * (nr + na) + 8), (2, 40 * (nr + na) + 8)):      # many and few k-mers in both
        rng = np.random.default_rng(seed)
        pool = np.arange(space, dtype=np.uint64) * np.uint64(3)
        rk = np.sort(rng.choice(pool, size=nr, replace=False))
        ak = np.sort(rng.choice(pool, size=na, replace=False))
        _walk_is_plain(m, rk, rng.integers(1, 2000, size=nr).astype(np.uint32), ak, rng.integers(1, 9, size=na).astype(np.uint32))
    if nr == na:                                                   # identical runs: every k-mer in both
        _walk_is_plain(m, rk, np.arange(1, nr + 1, dtype=np.uint32), rk, np.full(nr, 2, dtype=np.uint32))


def test_host_walk_owns_every_boundary_pair_once():
    m = _mfx()
    per, tile = m.db_join_grain()
    for grain in (per, tile):
        for shift in (0, 1, 2, grain - 1):
            rk, ak = boundary_world(grain, shift, 3 * tile + 5 * per + 3, seed=shift)
            assert len(np.intersect1d(rk, ak)) >= 3 * tile // grain
            _walk_is_plain(m, rk, (100 + np.arange(len(rk))).astype(np.uint32), ak, (1 + np.arange(len(ak)) % 7).astype(np.uint32))
