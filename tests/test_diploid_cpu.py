"""What of -diploid (mfx_db_diploid, csrc/mfx_diploid.h, `merfin -diploid`) needs no device: the text the kernels run -- role tag, merge of
the two assemblies, head compaction into the pair run, the tiled lane walk with a 64-bit asm value, the class rule, counters and piece sums
-- as mfx_db_diploid_host runs it, against the numpy reference of tests/diploid_ref.py, every field with ==; a k-mer of all three inputs on
every lane and tile boundary of the join's and of the pair step's merged order; the same text under AddressSanitizer + UBSan as a
stand-alone program (tools/native/diploid_sanitize.cpp); the class image's text form; the refusals of the API that come before any device is
looked at; and the argument errors of the CLI flag."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import diploid_ref as dr
from tests import stream_worlds as sw
from tests.test_join_cpu import boundary_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "merfin_amd", "bin", "merfin")
TOP = 2**32 - 1
BIG = 3 * 4096 + 17
SIZES = (0, 1, 7, 2047, 2048, 4095, 4097, BIG)
PROB = ([1, 1, 2, 0, 3, 3, 5], [0.5, 1.0, 0.25, 0.0, 0.75, 1.0, 0.125])      # rows for read counts 1 .. 7, a probK of 0 among them
EMPTY = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))


def _mfx():
    import merfin_amd as m
    return m


def asm_counts(n, seed):
    """assembly counts as assemblies have them: mostly 1 to 3, some above any -copies, escapes of both widths"""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 4, size=n).astype(np.uint32)
    if n:
        v[::11] = rng.integers(5, 40, size=len(v[::11])).astype(np.uint32)
        v[3::701] = np.uint32(2**22 - 1)
        v[5::907] = np.uint32(TOP)
    return v


def read_counts(n, seed):
    v = sw.mixed_counts(n, seed).copy()
    if n:
        v[1::9] = (1000 + np.arange(len(v[1::9])) * 7).astype(np.uint32)      # both sides of 1024 (the readK table), of 2048 and of 10000
        v[2::9] = 3
        v[4::503] = np.uint32(2**22 - 1)
        v[6::811] = np.uint32(TOP)
    return v


def three(k, sizes, seed):
    """(reads, hap1, hap2) of the sizes asked for, drawn from one pool of about twice the largest: every membership pattern turns up"""
    rng = np.random.default_rng(1000 * k + seed)
    pool = sw.random_keys(k, min(2 * max(sizes) + 8, 4 ** k), 77 * k + seed)
    out = []
    for i, n in enumerate(sizes):
        keys = np.sort(rng.choice(pool, size=n, replace=False))
        out.append((keys, read_counts(n, seed + i) if i == 0 else asm_counts(n, seed + i)))
    return tuple(out)


def sized_worlds():
    """every size in every role, the others' sizes turning through the list"""
    return [tuple(SIZES[(i + r * s) % len(SIZES)] for r in range(3)) for s in (1, 3) for i in range(len(SIZES))]


def diploid_boundary_world(grain, shift, total, order, k=21, seed=0):
    """boundary_world with a third input.  order "join": the k-mers of the reads and of the pair run (hap1 | hap2) alternate, a k-mer of all
    three where (p + shift) % grain == grain - 1 in the JOIN's merged order; "pair": the same for hap1 and hap2 in the PAIR STEP's merged order,
    the reads holding those k-mers and some others.  Returns (reads, hap1, hap2) as (k-mers, counts)."""
    ai, bi = boundary_world(grain, shift, total, seed=seed)
    both = np.intersect1d(ai, bi)
    if order == "join":
        rest = np.setdiff1d(bi, both)
        ri = ai
        h1 = np.union1d(both, rest[np.arange(len(rest)) % 3 != 1])
        h2 = np.union1d(both, rest[np.arange(len(rest)) % 3 != 0])
    else:
        h1, h2 = ai, bi
        top = int(max(ai.max(), bi.max()))
        ri = np.union1d(np.union1d(both, ai[::3]), np.union1d(bi[1::4], np.arange(top + 1, top + 40, dtype=np.uint64)))
    pool = sw.random_keys(k, int(max(ri.max(), h1.max(), h2.max())) + 1, 50 + seed)      # ascending: the world's order, over every piece
    ks = [pool[x.astype(np.int64)] for x in (ri, h1, h2)]
    return ((ks[0], (1 + np.arange(len(ks[0])) % 900).astype(np.uint32)), (ks[1], (1 + np.arange(len(ks[1])) % 5).astype(np.uint32)),
            (ks[2], (1 + np.arange(len(ks[2])) % 7).astype(np.uint32)))


def assert_boundaries_hit(world, grain, shift, order):
    """the merged positions, computed here: every multiple of `grain` inside the merged order has a k-mer of all three inputs whose first record
    stands at boundary - 1 - shift (shift 0: the boundary falls between the twins; 1: just behind the pair; grain - 1: just in front)"""
    (rk, _), (k1, _), (k2, _) = world
    a, b = (rk, np.union1d(k1, k2)) if order == "join" else (k1, k2)
    triple = np.intersect1d(np.intersect1d(rk, k1), k2)
    first = set((np.searchsorted(a, triple) + np.searchsorted(b, triple)).tolist())      # a's record of a k-mer stands in front of b's
    n = len(a) + len(b)
    bounds = list(range(grain, n - 1, grain))
    assert bounds, (grain, n)
    missed = [x for x in bounds if x - 1 - shift >= 0 and (x - 1 - shift) not in first]
    assert not missed, (order, grain, shift, missed[:5])
    return len(bounds)


def boundary_cases():
    m = _mfx()
    per, tile = m.db_join_grain()
    assert (per, tile) == (8, 2048)
    return [(order, grain, shift) for order in ("join", "pair") for grain in (per, tile) for shift in (0, 1, grain - 1)]


def _same(m, world, k, **kw):
    got = m.db_diploid_host(*world, k, copies=kw.get("copies", 4), max_mult=kw.get("max_mult", 10000), min_count=kw.get("lo", 0), max_count=kw.get("hi", TOP),
                            kparams=None if kw.get("peak") is None else m.KParams(kw["peak"], *(kw.get("prob") or (None, None))))
    want = dr.diploid(*world, k, **kw)
    what = (k, [len(x[0]) for x in world], kw)
    assert dr.same(got, want) is None, (dr.same(got, want), what)
    for g, w in zip(got["kmers"], want["kmers"]):                 # one (k-mer, r, c1, c2) per k-mer of the union, in ascending order
        assert np.array_equal(g.astype(np.uint64), w), what
    st = got["stats"]
    assert st["hap1"]["distinct"] == st["n_hap1"] == len(world[1][0]) and st["hap2"]["distinct"] == st["n_hap2"] == len(world[2][0]), what
    assert np.array_equal(got["asm_img"].sum(axis=0), got["cn_img"].sum(axis=0)), what
    return got


@pytest.mark.parametrize("k", [13, 21, 31])
def test_host_walk_against_numpy(k):
    m = _mfx()
    seen = set()
    for i, sizes in enumerate(sized_worlds()):
        world = three(k, sizes, i)
        _same(m, world, k, peak=17.3, prob=PROB if i % 2 else None)
        if i % 4 == 0:
            _same(m, world, k, copies=1, max_mult=4, lo=2, hi=50)
            _same(m, world, k, copies=6, max_mult=2048, lo=5, hi=40, peak=1.0)
        u = np.union1d(np.union1d(world[0][0], world[1][0]), world[2][0])
        seen |= set((np.isin(u, world[0][0]) * 4 + np.isin(u, world[1][0]) * 2 + np.isin(u, world[2][0])).tolist())
    assert seen == set(range(1, 8))                                # the seven membership patterns


def test_host_walk_edges():
    m = _mfx()
    top = np.array([5, 2**62 - 2, 2**62 - 1], dtype=np.uint64)     # k = 31: the tagged key uses all 64 bits
    full = np.full(3, TOP, dtype=np.uint32)
    got = _same(m, ((top[1:], full[1:]), (top, full), (top, full)), 31, peak=17.3)      # c1 = c2 = 2^32 - 1: cb clamps
    assert got["stats"]["both"]["total"] == 3 * TOP and got["stats"]["hap1"]["total"] == 3 * TOP and got["stats"]["both"]["only_total"] == TOP
    assert got["cn_img"][5, 10000] == 2 and got["cn_img"][5, 0] == 1 and got["asm_img"][3].sum() == 3
    _same(m, (EMPTY, EMPTY, EMPTY), 21, peak=17.3)
    a = three(21, (4097, 4097, 7), 3)
    got = _same(m, (a[0], a[1], a[1]), 21, peak=17.3)              # the same assembly twice: nothing is specific to either
    assert got["asm_img"][1].sum() == 0 and got["asm_img"][2].sum() == 0 and got["stats"]["n_shared"] == 4097
    lo = _same(m, a, 21, lo=2, hi=50)                              # -min / -max move the images and `found`, not the QV counters
    raw = _same(m, a, 21)
    for x in dr.NAMES:
        assert all(lo["stats"][x][f] == raw["stats"][x][f] for f in ("distinct", "total", "only_distinct", "only_total"))
    assert lo["stats"]["both"]["found"] < raw["stats"]["both"]["found"] and not np.array_equal(lo["cn_img"], raw["cn_img"])
    _same(m, ((np.array([0, 3, 5, 9, 15], dtype=np.uint64), np.array([20, 1, 2000, 7, 40], dtype=np.uint32)),
              (np.array([3, 4, 9], dtype=np.uint64), np.array([1, 2, 9], dtype=np.uint32)), (np.array([9, 14, 15], dtype=np.uint64), np.array([1, 1, 1], dtype=np.uint32))),
          2, peak=10.0, copies=2, max_mult=50)                     # 2k < 6: the piece is the k-mer itself
    for bad in (dict(copies=0), dict(copies=7), dict(max_mult=3), dict(max_mult=65537)):
        with pytest.raises(m.MfxError) as e:
            m.db_diploid_host(*a, 21, **bad)
        assert e.value.code == -1 and "is outside [" in str(e.value)


@pytest.mark.parametrize("case", range(12))
def test_host_walk_owns_every_boundary_kmer_once(case):
    m = _mfx()
    order, grain, shift = boundary_cases()[case]
    per, tile = m.db_join_grain()
    world = diploid_boundary_world(grain, shift, 3 * tile + 5 * per + 3, order, seed=shift)
    assert assert_boundaries_hit(world, grain, shift, order) >= 3 * tile // grain
    _same(m, world, 21, peak=1.0, copies=6, max_mult=1000)


def test_diploid_host_text_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "diploid_sanitize")
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "merfin_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "native", "diploid_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches, " in r.stdout and "MISMATCH" not in r.stdout


def test_asm_text(tmp_path):
    m = _mfx()
    img = np.zeros((4, 17), dtype=np.uint64)
    img[0, 1], img[1, 0], img[1, 9], img[2, 16], img[3, 2] = 500, 40, 2**40, 7, 3
    want = "Assembly\tkmer_multiplicity\tCount\nread-only\t1\t500\nhap1-only\t0\t40\nhap1-only\t9\t%d\nhap2-only\t16\t7\nshared\t2\t3\n" % 2**40
    m.diploid_write_asm(img, str(tmp_path / "a.hist"))
    assert (tmp_path / "a.hist").read_text() == want
    m.diploid_write_asm(img, str(tmp_path / "a.hist.gz"))
    assert gzip.open(str(tmp_path / "a.hist.gz"), "rt").read() == want
    m.diploid_write_asm(np.zeros((4, 5), dtype=np.uint64), str(tmp_path / "none.hist"))
    assert (tmp_path / "none.hist").read_text() == "Assembly\tkmer_multiplicity\tCount\n"
    assert m.DIPLOID_CLASSES == ("read-only", "hap1-only", "hap2-only", "shared")
    with pytest.raises(m.MfxError):
        m.diploid_write_asm(np.zeros((4, 3), dtype=np.uint64), str(tmp_path / "short.hist"))      # max_mult = 2
    with pytest.raises(m.MfxError):
        m.diploid_write_asm(img, str(tmp_path / "no_such_dir" / "a.hist"))


# ---- the API: refused before a device is touched (this machine has none: a call that went on would end in a HIP error)

def _write(m, path, k, n, seed):
    keys = sw.random_keys(k, n, seed)
    m.db_write_flat(str(path), k, keys, sw.mixed_counts(len(keys), seed))
    return str(path)


def _refused(m, call, code, text):
    with pytest.raises(m.MfxError) as e:
        call()
    assert e.value.code == code and text in str(e.value), str(e.value)
    assert "hip" not in str(e.value).lower()


def test_api_refusals(tmp_path, monkeypatch):
    m = _mfx()
    a = _write(m, tmp_path / "a.mfxk", 21, 4097, 1)
    b = _write(m, tmp_path / "b.mfxk", 21, 500, 2)
    k15 = _write(m, tmp_path / "k15.mfxk", 15, 500, 3)

    def every_role(bad, code, text):
        _refused(m, lambda: m.db_diploid(bad, a, b), code, text)
        _refused(m, lambda: m.db_diploid(a, bad, b, kparams=17.3), code, text)
        _refused(m, lambda: m.db_diploid(a, b, bad), code, text)

    _refused(m, lambda: m.db_diploid(a, k15, b), -1, "'%s' holds 15-mers, '%s' 21-mers: the inputs are of one k" % (k15, a))
    _refused(m, lambda: m.db_diploid(a, b, k15), -1, "the inputs are of one k")
    _refused(m, lambda: m.db_diploid(k15, a, b), -1, "the inputs are of one k")
    k32 = str(tmp_path / "k32.mfxk")
    m.db_write_flat(k32, 32, np.array([1, 5, 9], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint32))
    every_role(k32, -1, "'%s' holds 32-mers: the sorted join takes k <= 31" % k32)
    placed = str(tmp_path / "placed.mfxk")
    x, rc = sw.random_keys(21, 500, 9), np.zeros(500, dtype=np.uint64)
    fwd = x.copy()
    for _ in range(21):                                            # a placed database holds canonical k-mers
        rc = (rc << np.uint64(2)) | ((x & np.uint64(3)) ^ np.uint64(2))
        x = x >> np.uint64(2)
    canon = np.unique(np.minimum(fwd, rc))
    m.db_write_flat(str(tmp_path / "canon.mfxk"), 21, canon, np.ones(len(canon), dtype=np.uint32))
    m.db_convert_placed(str(tmp_path / "canon.mfxk"), placed)
    every_role(placed, -7, "'%s' is a placed database" % placed)
    monkeypatch.setenv("MFX_FLAT_DELTA", "0")
    packed = _write(m, tmp_path / "packed.mfxk", 21, 300, 4)
    monkeypatch.delenv("MFX_FLAT_DELTA")
    every_role(packed, -7, "'%s' is a packed flat file, not a sorted one: run `merfin -convert` first" % packed)
    plain = str(tmp_path / "plain.mfxk")
    m.db_write_flat(plain, 21, np.array([9, 5, 1], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint32))      # (not ascending: no sorted form)
    every_role(plain, -7, "flat file, not a sorted one: run `merfin -convert` first")
    text = tmp_path / "print.txt"
    text.write_text("ACGTACGTACGTACGTACGTA\t3\n")
    every_role(str(text), -7, "is not a flat k-mer file (`meryl print` text?)")
    (tmp_path / "db.meryl").mkdir()
    every_role(str(tmp_path / "db.meryl"), -7, "is a meryl directory")
    every_role(str(tmp_path / "absent.mfxk"), -6, "does not exist")
    for kw, what in ((dict(copies=0), "copies = 0 is outside [1, 6]"), (dict(copies=7), "copies = 7 is outside [1, 6]"), (dict(max_mult=3), "max_mult = 3 is outside [4, 65536]"),
                     (dict(max_mult=65537), "max_mult = 65537 is outside [4, 65536]")):
        _refused(m, lambda: m.db_diploid(a, b, b, **kw), -1, what)


def test_api_nulls_leave_the_outputs(tmp_path):
    from merfin_amd.binding import DbDiploidStats, DbJoinOpts
    m = _mfx()
    L = m.load_library()
    a = _write(m, tmp_path / "a.mfxk", 21, 100, 1).encode()
    o = DbJoinOpts(0, 0, TOP, 20.0, 0, None, None, 4, 100)
    img, cn = np.full(4 * 101, 77, dtype=np.uint64), np.full(6 * 101, 78, dtype=np.uint64)
    t, u = np.full(64, -1.0), np.full(192, -2.0)
    n, st = C.c_uint64(79), DbDiploidStats()
    st.solid = 80
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    ip, cp, tp, up = img.ctypes.data_as(u64p), cn.ctypes.data_as(u64p), t.ctypes.data_as(f64p), u.ctypes.data_as(f64p)
    full = [a, a, a, C.byref(o), ip, cp, C.byref(n), C.byref(st), tp, up]
    for i in range(8):                                             # every pointer but the two optional ones
        args = list(full)
        args[i] = None
        assert L.mfx_db_diploid(*args) == -1 and b"null argument" in L.mfx_last_error(), i
    for i in (8, 9):                                               # the piece sums: both or neither
        args = list(full)
        args[i] = None
        assert L.mfx_db_diploid(*args) == -1 and b"given together or not at all" in L.mfx_last_error()
    o.n_prob = 3                                                   # a -prob table announced and not given
    assert L.mfx_db_diploid(*full) == -1 and b"null argument" in L.mfx_last_error()
    absent = list(full)
    o.n_prob = 0
    absent[1] = str(tmp_path / "absent.mfxk").encode()
    assert L.mfx_db_diploid(*absent) == -6
    assert (img == 77).all() and (cn == 78).all() and (t == -1.0).all() and (u == -2.0).all() and n.value == 79 and st.solid == 80
    assert L.mfx_diploid_write_asm(None, 100, a) == -1 and L.mfx_diploid_write_asm(ip, 100, None) == -1


# ---- the CLI flag

DIP = ["-diploid", "-readmers", "{T}/r.mfxk", "-hap1", "{T}/a.mfxk", "-hap2", "{T}/b.mfxk", "-output", "{T}/o"]
SEPARATE = "-diploid, -trio, -histogram, -bin, -phase, -count, -convert and -merge are separate operations: give one of them."

CLI_CASES = [
    (["-diploid", "-hap1", "{T}/a.mfxk", "-hap2", "{T}/b.mfxk", "-output", "{T}/o"], ["-diploid needs the read database: give -readmers <file>."]),
    (["-diploid", "-readmers", "{T}/r.mfxk", "-hap2", "{T}/b.mfxk", "-output", "{T}/o"], ["-diploid needs the first assembly's database: give -hap1 <file>."]),
    (["-diploid", "-readmers", "{T}/r.mfxk", "-hap1", "{T}/a.mfxk", "-output", "{T}/o"], ["-diploid needs the second assembly's database: give -hap2 <file>."]),
    (DIP + ["-readmers", "{T}/a.mfxk"], ["-diploid takes one read database: -readmers was given more than once."]),
    (DIP + ["-hap1", "{T}/b.mfxk"], ["-diploid takes two assemblies: -hap1 was given more than once."]),
    (DIP + ["-hap2", "{T}/b.mfxk"], ["-diploid takes two assemblies: -hap2 was given more than once."]),
    (DIP[:-2], ["-diploid writes <output>.spectra-asm.hist, .spectra-cn.hist, .qv and .completeness.stats: give -output <stem>."]),
    (DIP + ["-sequence", "{T}/x.fa"], ["-diploid joins databases: it does not take -sequence (merfin -count -reads hap1.fasta -k K -output h1.mfxk, then -hap1 h1.mfxk)."]),
    (DIP + ["-seqmers", "{T}/a.mfxk"], ["-diploid takes its assemblies as -hap1 and -hap2: it does not take -seqmers."]),
    (DIP + ["-reads", "{T}/x.fa"], ["-diploid joins databases: it does not take -reads (count them first: -count)."]),
    (DIP + ["-hapmers", "{T}/a.mfxk"], ["-diploid compares assemblies with the reads: it does not take -hapmers (-phase and -bin do)."]),
    (DIP + ["-devices", "0"], ["-diploid runs on one device: it does not take -devices (-device d)."]),
    (DIP + ["-peak", "auto"], ["-diploid does not take -peak auto: the peak is read off a table, and -diploid builds none; give -peak <number>."]),
    (DIP + ["-spectrum"], ["-diploid is an operation of its own: it does not take a report type (-hist, -dump, -completeness, -spectrum, ...)."]),
    (DIP + ["-join"], ["-join is a way to run -completeness and -spectrum: -diploid is a join already and does not take it."]),
    (DIP + ["-trio"], [SEPARATE]),
    (DIP + ["-count"], [SEPARATE]),
    (DIP + ["-prob", "{T}/p.csv"], ["-prob belongs to the completeness report of -peak: give -peak <number> with it."]),
    (["-hap1", "{T}/a.mfxk", "-completeness", "-peak", "9", "-readmers", "{T}/r.mfxk", "-seqmers", "{T}/b.mfxk"],
     ["-hap1 and -hap2 name the assemblies of -diploid; they have no meaning without -diploid."]),
    (["-diploid", "-readmers", "{T}/r.mfxk", "-hap1", "{T}/a.mfxk", "-hap2", "{T}/none.mfxk", "-output", "{T}/o", "-copies", "9"],
     ["Invalid -copies '9': an integer from 1 to 6.", "Cannot read the -hap2 database '{T}/none.mfxk'."]),
]


@pytest.mark.parametrize("case", range(len(CLI_CASES)))
def test_cli_refusal(tmp_path, case):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    for name in ("r.mfxk", "a.mfxk", "b.mfxk", "x.fa", "p.csv"):
        (tmp_path / name).write_text(">r0\nACGTACGTACGTACGTACGTACGTACGT\n")      # (refused before a file is opened)
    argv, lines = CLI_CASES[case]
    r = subprocess.run([EXE] + [a.replace("{T}", str(tmp_path)) for a in argv], capture_output=True, text=True)
    assert r.returncode == 1, r.stderr
    assert r.stderr.startswith("usage: ")
    # the usage text, the entry of -diploid behind it, then the lines of this command line
    head, sep, tail = r.stderr.partition("  Two haplotype assemblies against the reads (an operation of its own: no -sequence, no -seqmers):\n")
    assert sep and "-diploid" not in head, r.stderr
    entry, _, mine = tail.partition("\n\n")
    assert "-hap1 db / -hap2 db" in entry and "unvalidated against Merqury" in entry and "-peak auto is not taken" in entry
    assert mine.splitlines() == [l.replace("{T}", str(tmp_path)) for l in lines], r.stderr
    assert "ERROR: HIP device" not in r.stderr                    # refused before a device is asked for
    assert not any(os.path.exists(str(tmp_path / ("o" + s))) for s in (".spectra-asm.hist", ".spectra-cn.hist", ".qv", ".completeness.stats"))


def test_usage_without_diploid_is_unchanged():
    """a command line that names neither -diploid nor a flag of its own gets the usage text as it was"""
    for argv in (["-bogus"], ["-completeness", "-join", "-readmers", "x"], ["-trio"]):
        r = subprocess.run([EXE] + argv, capture_output=True, text=True)
        assert r.returncode == 1 and "-diploid" not in r.stderr and "-hap1" not in r.stderr, argv
