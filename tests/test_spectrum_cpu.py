"""The host side of the copy-number spectrum, without a device: mfx_spectrum_peak against the restatement of its rule with
fractions.Fraction (tests/spectrum_ref.py), the report writer byte for byte, and the refusals.  The kernels are checked on the
GPU (tests/test_gpu_spectrum.py)."""
import ctypes as C
import gzip
import math

import numpy as np
import pytest

import merfin_amd as m
from tests import spectrum_ref as sr
from tests import synth


def _both(row):
    """the C function's answer as the reference's tuple (or None), checked against the reference"""
    got = m.spectrum_peak(row)
    got = None if got is None else (got["valley"], got["main_peak"], got["haploid_peak"], got["count_at_peak"])
    assert got == sr.peak(row), (got, sr.peak(row))
    return got


def _pois(lam, n):
    return np.array([math.exp(-lam + i * math.log(lam) - math.lgamma(i + 1)) for i in range(n)])


WORLDS = [  # (k, peak, seed, sizes, expected (valley, main, haploid))
    (21, 17.3, 42, (120000, 9000, 4096, 4097, 500, 20, 0, 8191), (1, 17, 17)),
    (21, 26.0, 43, (120000, 9000, 4096, 4097, 500, 20, 0, 8191), (1, 26, 26)),
    (31, 17.3, 44, (60000, 20000, 4097, 30, 0), (1, 17, 17)),
    (15, 9.0, 45, None, (1, 9, 9)),
]


@pytest.mark.parametrize("k,peak,seed,sizes,want", WORLDS)
def test_peak_of_the_synthetic_worlds(k, peak, seed, sizes, want):
    kw = {} if sizes is None else {"sizes": sizes}
    _, read, asm = synth.world(k=k, peak=peak, seed=seed, **kw)
    row = sr.image(read, asm, 4, 10000)[1]
    got = _both(row)
    assert got is not None and got[:3] == want and got[3] == int(row[want[2]])


def test_peak_of_the_named_rows():
    M = 10000
    # a haploid assembly of a diploid genome: 1 : 3 of Poisson(26) and Poisson(52), geometric errors 10^6 * 0.3^m
    mix = 1e6 * (0.25 * _pois(26, M + 1) + 0.75 * _pois(52, M + 1)) + 1e6 * 0.3 ** np.arange(M + 1)
    row = np.floor(mix).astype(np.uint64)
    row[0] = 0
    assert _both(row)[:3] == (9, 52, 26)
    assert _both(np.floor(1e6 * _pois(2.5, M + 1)).astype(np.uint64)) is None                    # a peak too low to resolve
    assert _both(np.zeros(M + 1, dtype=np.uint64)) is None                                       # empty
    assert _both(np.array([0] + [10 ** 12 // i for i in range(1, M + 1)], dtype=np.uint64)) is None     # falls all the way


def test_peak_of_random_rows():
    r = np.random.default_rng(20261018)
    found = 0
    for i in range(300):
        M = (4, 5, 50, 1024, 65536)[i % 5]
        n = int(r.integers(200, 200001))
        lam = float(r.uniform(1.5, min(400, max(3.0, M * 0.8))))
        w2 = float(r.uniform(0, 1)) if i % 3 else 0.0          # share of the 2-copy component
        cells = r.poisson(np.where(r.random(n) < w2, 2 * lam, lam))
        if (i // 5) % 2:                                        # an error slope
            cells = np.concatenate([cells, r.geometric(float(r.uniform(0.3, 0.8)), size=n // 3)])
        row = np.bincount(np.minimum(cells, M), minlength=M + 1).astype(np.uint64)
        found += _both(row) is not None
    assert 30 < found < 300                                     # both endings of the rule are exercised


def test_peak_edges():
    M = 100
    row = np.zeros(M + 1, dtype=np.uint64)
    row[0] = 10 ** 9
    assert _both(row) is None                                   # mass in column 0 only: it takes no part
    row[:] = 0
    row[M] = 10 ** 9
    assert _both(row) is None                                   # ... nor does the overflow column
    # ties at the maximum: two equal humps, the smaller m wins; a plateau
    row[:] = 0
    row[30] = row[60] = 1000
    assert _both(row)[:3] == (1, 28, 28)
    row[:] = 0
    row[20:70] = 7
    got = _both(row)
    assert got is not None and got[1] == 22
    # a lone cell at either end of the range that takes part
    for at in (1, 2, M - 1):
        row[:] = 0
        row[at] = 5
        _both(row)
    # cells of 2^63: window sums beyond 64 bits, compared in 128
    row[:] = 0
    row[1], row[2] = 2 ** 63, 2 ** 62
    row[40:45] = 2 ** 63
    row[42] = 2 ** 63 + 1
    row[20:23] = 2 ** 63 - 1
    got = _both(row)
    assert got is not None and got[1] == 42
    row = np.full(M + 1, 2 ** 64 - 1, dtype=np.uint64)
    _both(row)
    for M in (4, 5):
        for cells in ((0, 5, 1, 9, 0), (0, 1, 2, 3, 0), (0, 3, 2, 1, 9), (7, 0, 0, 1, 7)):
            _both(np.array(list(cells) + [0] * (M - 4), dtype=np.uint64))


IMG = np.zeros((3, 6), dtype=np.uint64)         # copies = 1, max_mult = 5
IMG[0, 1], IMG[0, 5] = 12, 3
IMG[1, 0], IMG[1, 4], IMG[1, 5] = 7, 2 ** 40, 1
IMG[2, 2], IMG[2, 5] = 9, 2 ** 64 - 1
TEXT1 = ("Copies\tkmer_multiplicity\tCount\n" "read-only\t1\t12\n" "read-only\t5\t3\n" "1\t0\t7\n" "1\t4\t1099511627776\n" "1\t5\t1\n"
         ">1\t2\t9\n" ">1\t5\t18446744073709551615\n")
TEXT0 = "Copies\tkmer_multiplicity\tCount\n" "1\t0\t7\n" "1\t4\t1099511627776\n" "1\t5\t1\n" ">1\t2\t9\n" ">1\t5\t18446744073709551615\n"


def test_writer_byte_for_byte(tmp_path):
    p = str(tmp_path / "a.spectra-cn.hist")
    m.spectrum_write(IMG, p, with_read_only=True)
    assert open(p).read() == TEXT1 == sr.text(IMG, True)
    m.spectrum_write(IMG, p, with_read_only=False)
    assert open(p).read() == TEXT0 == sr.text(IMG, False)
    z = str(tmp_path / "a.spectra-cn.hist.gz")
    m.spectrum_write(IMG, z)
    assert gzip.open(z, "rt").read() == TEXT1
    # the ">C" label carries the number of copies; an all-zero image is the header alone
    img = np.zeros((8, 5), dtype=np.uint64)
    img[7, 4] = 1
    img[6, 3] = 2
    m.spectrum_write(img, p)
    assert open(p).read() == "Copies\tkmer_multiplicity\tCount\n6\t3\t2\n>6\t4\t1\n"
    m.spectrum_write(np.zeros((8, 5), dtype=np.uint64), p)
    assert open(p).read() == "Copies\tkmer_multiplicity\tCount\n"


def test_refusals(tmp_path):
    L = m.load_library()
    u64p = C.POINTER(C.c_uint64)
    buf = (C.c_uint64 * 16)()
    from merfin_amd import binding
    out = binding._SpectrumPeak()
    for row, mm in ((buf, 3), (buf, 65537), (None, 10)):
        assert L.mfx_spectrum_peak(C.cast(row, u64p), mm, C.byref(out)) == -1 and L.mfx_last_error()
    assert L.mfx_spectrum_peak(C.cast(buf, u64p), 10, None) == -1
    p = str(tmp_path / "x").encode()
    for copies, mm in ((0, 10), (7, 10), (4, 3), (4, 65537)):
        assert L.mfx_spectrum_write(C.cast(buf, u64p), copies, mm, 1, p) == -1
        assert b"outside" in L.mfx_last_error()
    assert L.mfx_spectrum_write(None, 1, 4, 1, p) == -1 and L.mfx_spectrum_write(C.cast(buf, u64p), 1, 4, 1, None) == -1
    assert L.mfx_spectrum_write(C.cast(buf, u64p), 1, 4, 1, str(tmp_path / "no" / "dir" / "x").encode()) == -6
    # mfx_spectrum_run checks its arguments before it touches the index or a device
    n = C.c_uint64(0)
    assert L.mfx_spectrum_run(None, 4, 100, C.cast(buf, u64p), C.byref(n)) == -1
    with pytest.raises(m.MfxError):
        m.spectrum_peak(np.zeros(3, dtype=np.uint64))
