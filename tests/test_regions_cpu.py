"""What of -regions (mfx_regions_run, csrc/mfx_regions.h) needs no device: the steps between its two passes -- run starts and ends
per 64-bit word of a class plane, count, scan, scatter, the joining over gaps, the filter, the records' order -- as
mfx_regions_from_planes_host runs them on the host (the text the plane kernels run) against the numpy pipeline of
tests/regions_ref.py on hand-made planes; the same text under AddressSanitizer + UBSan as a stand-alone program
(tools/native/regions_sanitize.cpp); and the refusals of the API that come before any device is looked at."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import regions_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 21
GAPS = (0, 1, K - 1, 64, 4096, 10**6)
MINS = (1, K, 1000)


def _mfx():
    import merfin_amd as m
    return m


def _empty(lens):
    return [tuple(np.zeros(n, dtype=bool) for _ in range(3)) for n in lens]


def _worlds():
    out = {}
    lens = (3 * 4096 + 77,)
    m = _empty(lens)
    for i, p in enumerate((0, 63, 64, 4095, 4096, lens[0] - 1)):
        m[0][i % 3][p] = True
    out["single bits"] = (lens, m)
    lens = (2 * 4096 + 5,)
    m = _empty(lens)
    m[0][0][64:128] = True                    # a full word
    m[0][0][192:384] = True                   # three full words
    m[0][1][60:70] = True                     # over a word edge
    m[0][1][250:262] = True
    m[0][1][4090:4100] = True                 # over a tile edge
    m[0][2][100:300] = True                   # a run spanning more than three words, unaligned
    m[0][2][8190:8197] = True                 # up to the contig's last position
    out["words and edges"] = (lens, m)
    lens = (9000,)
    m = _empty(lens)
    m[0][0][::2] = True                       # alternating bits
    m[0][1][:] = True                         # every word full
    out["alternating and full"] = (lens, m)
    lens = (4096, 8192, 0, 10, 4097, 1)
    m = _empty(lens)
    m[0][0][4000:] = True                     # contig 0 ends flagged in its tile's last bit ...
    m[1][0][:50] = True                       # ... and contig 1 starts flagged in the next word
    m[1][0][8100:] = True
    m[3][0][:] = True
    m[4][0][:3] = True
    m[4][0][4096] = True
    m[5][0][0] = True
    m[0][2][4095] = True
    m[1][2][0] = True
    out["contigs that touch"] = (lens, m)
    r = np.random.default_rng(17)
    lens = (4097, 64, 12288, 63)
    m = [tuple(np.cumsum(r.random(n) < 0.02) % 2 == 1 for _ in range(3)) for n in lens]
    out["random"] = (lens, m)
    return out


WORLDS = _worlds()


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_planes_to_regions_on_the_host(name):
    m = _mfx()
    lens, masks = WORLDS[name]
    planes = rr.planes_of(masks, lens)
    for gap in GAPS:
        for mk in MINS:
            want = rr.regions_from_masks(masks, gap, mk)
            got = m.regions_from_planes_host(planes, lens, gap, mk)
            assert got.dtype == m.REGION_DTYPE and got.dtype.itemsize == 56
            assert rr.device_records(got) == want, (name, gap, mk)
    if name == "contigs that touch":
        # nothing joins across a contig's end, whatever the gap
        for gap in GAPS:
            got = rr.device_records(m.regions_from_planes_host(planes, lens, gap, 1))
            assert {"contig": 0, "cls": 0, "start": 4000, "end": 4096, "n_kmers": 96, "sum_readK": 0, "sum_asmK": 0, "ext_kstar": 0.0} in got
            assert [r for r in got if r["contig"] == 1 and r["cls"] == 0][0]["start"] == 0
            assert [r for r in got if r["cls"] == 2] == [
                {"contig": 0, "cls": 2, "start": 4095, "end": 4096, "n_kmers": 1, "sum_readK": 0, "sum_asmK": 0, "ext_kstar": 0.0},
                {"contig": 1, "cls": 2, "start": 0, "end": 1, "n_kmers": 1, "sum_readK": 0, "sum_asmK": 0, "ext_kstar": 0.0}]
    if name == "alternating and full":
        got = rr.device_records(m.regions_from_planes_host(planes, lens, 0, 1))
        assert sum(r["cls"] == 0 for r in got) == 4500 and sum(r["cls"] == 1 for r in got) == 1
        got = rr.device_records(m.regions_from_planes_host(planes, lens, 1, 1))
        assert [r for r in got if r["cls"] == 0] == [{"contig": 0, "cls": 0, "start": 0, "end": 8999, "n_kmers": 4500, "sum_readK": 0, "sum_asmK": 0, "ext_kstar": 0.0}]


def test_host_planes_refusals():
    m = _mfx()
    lens = (100,)
    planes = np.zeros((3, 64), dtype=np.uint64)
    assert len(m.regions_from_planes_host(planes, lens)) == 0
    planes[1, 1] = np.uint64(1) << np.uint64(36)              # position 100: beyond the contig's 100 positions
    with pytest.raises(m.MfxError) as e:
        m.regions_from_planes_host(planes, lens)
    assert e.value.code == -1 and "beyond the 100 positions of contig 0" in str(e.value)
    planes[1, 1] = np.uint64(1) << np.uint64(35)              # position 99: the last one
    assert rr.device_records(m.regions_from_planes_host(planes, lens))[0]["start"] == 99
    with pytest.raises(m.MfxError):
        m.regions_from_planes_host(np.zeros(5, dtype=np.uint64), lens)
    assert len(m.regions_from_planes_host(np.zeros(0, dtype=np.uint64), ())) == 0


def test_api_refusals_without_a_device():
    m = _mfx()
    L = m.load_library()
    from merfin_amd.binding import _RegionsOpts
    o = _RegionsOpts(1.0, 0, 1)
    h = C.c_void_p(None)
    assert L.mfx_regions_run(None, None, C.byref(o), C.byref(h), None, None) == -1
    assert b"mfx_regions_run: null argument" in L.mfx_last_error() and not h.value
    assert L.mfx_regions_count(None) == 0 and L.mfx_regions_tiles_revisited(None) == 0
    assert L.mfx_regions_copy(None, None, 0) == -1 and b"mfx_regions_copy" in L.mfx_last_error()
    assert L.mfx_regions_write(None, 0, None, None, 21, b"x.bed") == -1 and b"mfx_regions_write: null argument" in L.mfx_last_error()
    L.mfx_regions_free(None)
    n = C.c_uint64(0)
    assert L.mfx_regions_from_planes_host(None, None, 0, None, None, 0, C.byref(n)) == -1
    with pytest.raises(m.MfxError):
        m.binding._regions_opts(1.0, -1, 1)


def test_regions_host_text_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "regions_sanitize")
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "merfin_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "native", "regions_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches, " in r.stdout and "MISMATCH" not in r.stdout
