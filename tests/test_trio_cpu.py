"""What of -trio (mfx_db_trio, csrc/mfx_trio.h) needs no device: the class rule as mfx_db_trio_host runs it on the host -- the text the
kernels run: role tag, merge, head walk, rule, histogram columns -- against the numpy reference of tests/trio_ref.py, every field with ==;
the same text under AddressSanitizer + UBSan as a stand-alone program (tools/native/trio_sanitize.cpp); the histogram's text form; and the
refusals of mfx_db_trio, mfx_db_trio_hist and mfx_db_histogram that come before any device is looked at."""
import ctypes as C
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import stream_worlds as sw
from tests import trio_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = ((1, 1, 1), (2, 3, 2), (5, 5, 5))


def _mfx():
    import merfin_amd as m
    return m


def _same(m, mat, pat, child, cuts, max_mult):
    (ak, av), (bk, bv), img, st = m.db_trio_host(mat, pat, child, *cuts, max_mult=max_mult)
    (wak, wav), (wbk, wbv), wimg, wst = tr.reference(mat, pat, child, *cuts, max_mult=max_mult)
    what = (cuts, max_mult, len(mat[0]), len(pat[0]), None if child is None else len(child[0]))
    assert np.array_equal(ak, wak) and np.array_equal(av, wav) and np.array_equal(bk, wbk) and np.array_equal(bv, wbv), what
    assert ak.dtype == np.uint64 and av.dtype == np.uint32 and (img == wimg).all(), what
    assert {n: st[n] for n in tr.COUNTERS} == wst, what
    assert (st["cut_mat"], st["cut_pat"], st["cut_child"]) == (cuts[0], cuts[1], cuts[2] if child is not None else 0)
    return st


@pytest.mark.parametrize("with_child", [True, False])
@pytest.mark.parametrize("k", [15, 21, 31])
def test_host_rule_against_numpy(k, with_child):
    m = _mfx()
    seen = set()
    for case in range(7):                                     # every size in every role, then three databases that overlap widely
        mat, pat, child = tr.sets(k, tr.roles(case) if case < 6 else (20000, 4097, 4095), 500 + 10 * k + case, hi=8)
        for cuts in CUTS:
            for max_mult in (4, 10000):
                _same(m, mat, pat, child if with_child else None, cuts, max_mult)
        u = np.union1d(np.union1d(mat[0], pat[0]), child[0])
        seen |= set((np.isin(u, mat[0]) * 4 + np.isin(u, pat[0]) * 2 + np.isin(u, child[0])).tolist())
    assert seen == set(range(1, 8))                            # the seven membership patterns


def test_host_rule_edges():
    m = _mfx()
    top = np.array([2**62 - 2, 2**62 - 1], dtype=np.uint64)   # k = 31: the tagged key uses all 64 bits
    big = np.array([2**32 - 1, 2**32 - 1], dtype=np.uint32)
    st = _same(m, (top, big), (top[:1], big[:1]), (top, np.array([7, 2**32 - 2], dtype=np.uint32)), (2**32 - 1, 1, 2**32 - 2), 65536)
    assert (st["n_a"], st["n_b"], st["n_both"], st["n_child_cut"]) == (1, 0, 1, 1)
    _same(m, tr.EMPTY, tr.EMPTY, tr.EMPTY, (1, 1, 1), 4)
    _same(m, tr.EMPTY, tr.EMPTY, None, (1, 1, 1), 4)
    a = tr.sets(21, (4097,), 3)[0]
    st = _same(m, a, a, None, (1, 1, 1), 16)                   # equal parents: nothing is specific to either
    assert (st["n_a"], st["n_b"], st["n_both"]) == (0, 0, 4097)
    _same(m, a, tr.EMPTY, tr.EMPTY, (1, 1, 1), 16)             # a child of no k-mers: A is empty
    for bad in (dict(cut_mat=0, cut_pat=1), dict(cut_mat=1, cut_pat=0), dict(cut_mat=1, cut_pat=1, cut_child=0), dict(cut_mat=1, cut_pat=1, max_mult=3)):
        with pytest.raises(m.MfxError) as e:
            m.db_trio_host(a, a, a, **bad)
        assert e.value.code == -1


def test_trio_host_text_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "trio_sanitize")
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "merfin_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "native", "trio_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches, " in r.stdout and "MISMATCH" not in r.stdout


def test_histogram_text(tmp_path):
    m = _mfx()
    row = np.zeros(17, dtype=np.uint64)
    row[[1, 2, 9, 16]] = [500, 40, 2**40, 7]                  # (the overflow column is written as max_mult)
    want = "1\t500\n2\t40\n9\t%d\n16\t7\n" % 2**40
    m.db_histogram_write(row, str(tmp_path / "h.hist"))
    assert (tmp_path / "h.hist").read_text() == want
    m.db_histogram_write(row, str(tmp_path / "h.hist.gz"))
    assert gzip.open(str(tmp_path / "h.hist.gz"), "rt").read() == want
    m.db_histogram_write(np.zeros(5, dtype=np.uint64), str(tmp_path / "none.hist"))
    assert (tmp_path / "none.hist").read_text() == ""
    with pytest.raises(m.MfxError):
        m.db_histogram_write(np.zeros(3, dtype=np.uint64), str(tmp_path / "short.hist"))      # max_mult = 2
    with pytest.raises(m.MfxError):
        m.db_histogram_write(row, str(tmp_path / "no_such_dir" / "h.hist"))


# ---- the API: refused before a device is touched (this machine has none: a call that went on would end in a HIP error)

def _write(m, path, k, n, seed):
    keys = sw.random_keys(k, n, seed)
    m.db_write_flat(str(path), k, keys, sw.mixed_counts(len(keys), seed))
    return str(path)


def _refused(m, call, code, text, absent=()):
    with pytest.raises(m.MfxError) as e:
        call()
    assert e.value.code == code and text in str(e.value), str(e.value)
    assert "hip" not in str(e.value).lower()
    for p in absent:
        assert not os.path.exists(p) and not os.path.exists(p + ".blocks")


def test_api_refusals(tmp_path, monkeypatch):
    m = _mfx()
    a = _write(m, tmp_path / "a.mfxk", 21, 4097, 1)
    b = _write(m, tmp_path / "b.mfxk", 21, 500, 2)
    c = _write(m, tmp_path / "c.mfxk", 21, 700, 5)
    k15 = _write(m, tmp_path / "k15.mfxk", 15, 500, 3)
    oa, ob = str(tmp_path / "A.mfxk"), str(tmp_path / "B.mfxk")
    outs = (oa, ob)

    def every_role(bad, code, text):
        """the refused file as mat, as pat, as child, and alone"""
        _refused(m, lambda: m.db_trio(bad, b, c, oa, ob, cut_mat=1, cut_pat=1, cut_child=1), code, text, outs)
        _refused(m, lambda: m.db_trio(a, bad, None, oa, ob), code, text, outs)
        _refused(m, lambda: m.db_trio(a, b, bad, oa, ob), code, text, outs)
        _refused(m, lambda: m.db_trio_hist(a, bad, c, max_mult=100), code, text)
        _refused(m, lambda: m.db_histogram(bad, max_mult=100), code, text)

    _refused(m, lambda: m.db_trio(a, k15, None, oa, ob), -1, "'%s' holds 15-mers, '%s' 21-mers: the inputs are of one k" % (k15, a), outs)
    _refused(m, lambda: m.db_trio(a, b, k15, oa, ob), -1, "the inputs are of one k", outs)
    _refused(m, lambda: m.db_trio_hist(k15, b), -1, "the inputs are of one k")
    k32 = str(tmp_path / "k32.mfxk")
    m.db_write_flat(k32, 32, np.array([1, 5, 9], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint32))
    every_role(k32, -1, "'%s' holds 32-mers" % k32)
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
    # the outputs
    before = [open(p, "rb").read() for p in (a, b, c)]
    for i, (x_, y_) in enumerate(((a, ob), (oa, b), (c, ob), (oa, c))):
        _refused(m, lambda: m.db_trio(a, b, c, x_, y_, cut_mat=1, cut_pat=1, cut_child=1), -1, "is the input '%s'" % (a, b, c, c)[i])
    assert [open(p, "rb").read() for p in (a, b, c)] == before and not os.path.exists(oa) and not os.path.exists(ob)
    _refused(m, lambda: m.db_trio(a, b, None, oa, oa, cut_mat=1, cut_pat=1), -1, "are the same file", outs)
    os.link(a, str(tmp_path / "hard.mfxk"))                      # an output that is an input under another name
    _refused(m, lambda: m.db_trio(a, b, None, str(tmp_path / "hard.mfxk"), ob, cut_mat=1, cut_pat=1), -1, "is the input '%s'" % a)
    # the options
    _refused(m, lambda: m.db_trio(a, b, None, oa, ob, cut_mat=1, cut_pat=1, cut_child=2), -1, "cut_child = 2 without a child database", outs)
    for mm in (3, 65537):
        _refused(m, lambda: m.db_trio(a, b, c, oa, ob, max_mult=mm), -1, "max_mult = %d is outside [4, 65536]" % mm, outs)
        _refused(m, lambda: m.db_trio_hist(a, b, c, max_mult=mm), -1, "max_mult = %d is outside [4, 65536]" % mm)
        _refused(m, lambda: m.db_histogram(a, max_mult=mm), -1, "max_mult = %d is outside [4, 65536]" % mm)


def test_api_nulls(tmp_path):
    m = _mfx()
    from merfin_amd.binding import DbTrioOpts
    L = m.load_library()
    a = _write(m, tmp_path / "a.mfxk", 21, 100, 1).encode()
    oa, ob = str(tmp_path / "A.mfxk").encode(), str(tmp_path / "B.mfxk").encode()
    o = DbTrioOpts(1, 1, 0, 100, 0)
    img = (C.c_uint64 * (3 * 101))()
    for args in ((None, a, None, oa, ob, C.byref(o)), (a, None, None, oa, ob, C.byref(o)), (a, a, None, None, ob, C.byref(o)), (a, a, None, oa, None, C.byref(o)),
                 (a, a, None, oa, ob, None)):
        assert L.mfx_db_trio(*args, None, None) == -1 and b"null argument" in L.mfx_last_error()
    assert L.mfx_db_trio_hist(a, a, None, 100, None, None, 0) == -1 and b"null argument" in L.mfx_last_error()
    assert L.mfx_db_trio_hist(None, a, None, 100, img, None, 0) == -1
    assert L.mfx_db_histogram(None, 100, img, None, 0) == -1 and b"null argument" in L.mfx_last_error()
    assert L.mfx_db_histogram(a, 100, None, None, 0) == -1
    assert L.mfx_db_histogram_write(None, 100, oa) == -1 and L.mfx_db_histogram_write(img, 100, None) == -1
    assert not os.path.exists(oa.decode()) and not os.path.exists(ob.decode())
