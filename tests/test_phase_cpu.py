"""What of -phase (mfx_phase_run, csrc/mfx_phase.h) needs no device: pass 2 -- the carried marker, run starts per 64-bit word, the
marker ranks, long and short runs, block openings, block sums -- as mfx_phase_from_planes_host runs it on the host (the text the
plane kernels run) against the sequential walk of tests/phase_ref.py on hand-made planes; the three texts against the formatters;
the same text under AddressSanitizer + UBSan as a stand-alone program (tools/native/phase_sanitize.cpp); and the refusals of the
API that come before any device is looked at."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import phase_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 21
SWITCHES = (0, 1, 3, 100)
RANGES = (0, K, 64, 5000, 10**6)
A, B = 0, 1


def _mfx():
    import merfin_amd as m
    return m


def _stretch(p, hap, n, step=3):
    """n markers of one haplotype from p on, `step` apart -> (markers, the position behind them)"""
    return [(p + i * step, hap) for i in range(n)], p + n * step


def world(S, R):
    """every plane shape of the list, one contig each (names for the asserts below)"""
    lens, mk, names = [], [], []

    def add(name, n, markers):
        assert markers == sorted(markers) and len({p for p, _ in markers}) == len(markers) and all(p < n for p, _ in markers)
        names.append(name); lens.append(n); mk.append(markers)

    # bits 63 | 0 of adjacent words, positions 4095 | 4096: same and opposite haplotypes over the edge
    add("edges", 3 * 4096 + 77, [(63, A), (64, B), (127, B), (128, B), (191, A), (192, A), (4095, A), (4096, A), (8191, A), (8192, B), (3 * 4096 + 76, B)])
    # a run continued across 3 empty tiles; two runs of opposite haplotypes separated by 3 empty tiles
    add("empty tiles", 10 * 4096, [(100, A), (200, A), (4 * 4096 + 5, A), (4 * 4096 + 100, B), (8 * 4096 + 50, A), (9 * 4096 + 4095, A)])
    add("tile + 1", 4097, [(0, A), (4096, B)])
    # contigs of 0 positions and of fewer than k positions between others: nothing is carried over a contig's end
    add("ends flagged", 4096, [(4000, A), (4095, A)])
    add("no position", 0, [])
    add("shorter than k", 10, [])
    add("starts flagged", 8192, [(0, A), (1, B), (8191, B)])
    add("no marker", 5000, [])
    add("starts with the other", 4097, [(4096, A)])
    # only short runs (for S >= 1 and R >= k): the majority, and the tie
    add("short majority", 600, [(10, B), (50, A), (90, B), (130, A), (170, B)])
    add("short tie", 600, [(10, B), (50, A), (90, B), (130, A)])
    # alternating haplotypes at every marker for 200 markers
    add("alternating", 200 * 7 + 50, [(5 + 7 * i, i & 1) for i in range(200)])
    # an intrusion of exactly S and of S + 1 markers
    m, p = _stretch(7, A, S + 5)
    for n in (S, S + 1):
        x, p = _stretch(p, B, n); m += x
        x, p = _stretch(p, A, S + 5); m += x
    add("intrusions", p + K, m)
    # an intrusion of S markers whose span is exactly R and R + 1 (where S markers fit such a span)
    if S >= 2 and S - 1 <= R - K <= 10**6:
        m, p = _stretch(3, A, S + 5)
        for span in (R, R + 1):
            m += [(p + i, B) for i in range(S - 1)] + [(p + span - K, B)]
            p += span - K + 1
            x, p = _stretch(p, A, S + 5); m += x
        add("spans", p + K, m)
    # leading and trailing short runs
    m, p = _stretch(2, B, 1)
    x, p = _stretch(p, A, S + 5); m += x
    x, p = _stretch(p, B, 1); m += x
    add("leading and trailing", p + K, m)
    # short runs between two long runs of opposite haplotypes
    m, p = _stretch(0, A, S + 5)
    x, p = _stretch(p, B, 1); m += x
    x, p = _stretch(p, A, 1); m += x
    x, p = _stretch(p, B, S + 5); m += x
    x, p = _stretch(p, A, S + 5, step=70); m += x
    add("between long runs", p + K, m)
    return names, lens, mk


@pytest.mark.parametrize("S", SWITCHES)
@pytest.mark.parametrize("R", RANGES)
def test_planes_to_blocks_on_the_host(S, R):
    m = _mfx()
    names, lens, mk = world(S, R)
    planes = pr.planes_of(mk, lens)
    want = pr.blocks(mk, K, S, R)
    got = m.phase_from_planes_host(planes, lens, K, S, R)
    assert got.dtype == m.PHASE_DTYPE and got.dtype.itemsize == 48
    got = pr.device_records(got)
    for c, name in enumerate(names):
        assert [r for r in got if r["contig"] == c] == [r for r in want if r["contig"] == c], (name, S, R)
    assert got == want
    for c in range(len(lens)):                                # every marker is in exactly one block
        assert sum(r["n_hap"] + r["n_switch"] for r in got if r["contig"] == c) == len(mk[c])


def test_the_rule_on_known_cases():
    """the reference itself, on cases small enough to state by hand (S = 1, R = 5000 unless said)"""
    m = _mfx()
    names, lens, mk = world(1, 5000)
    got = pr.device_records(m.phase_from_planes_host(pr.planes_of(mk, lens), lens, K, 1, 5000))
    by = {name: [r for r in got if r["contig"] == c] for c, name in enumerate(names)}
    assert by["no marker"] == [] and by["no position"] == [] and by["shorter than k"] == []
    c = names.index("short majority")
    assert by["short majority"] == [{"contig": c, "hap": B, "start": 10, "end": 171, "n_hap": 3, "n_switch": 2, "n_switch_runs": 2}]
    c = names.index("short tie")
    assert by["short tie"] == [{"contig": c, "hap": A, "start": 10, "end": 131, "n_hap": 2, "n_switch": 2, "n_switch_runs": 2}]
    c = names.index("ends flagged")
    assert by["ends flagged"] == [{"contig": c, "hap": A, "start": 4000, "end": 4096, "n_hap": 2, "n_switch": 0, "n_switch_runs": 0}]
    assert by["starts flagged"][0]["start"] == 0 and by["starts with the other"][0]["n_hap"] == 1
    # an intrusion of S = 1 marker stays inside its block, one of 2 markers opens a block and the A run behind it another
    assert [(r["hap"], r["n_hap"], r["n_switch"], r["n_switch_runs"]) for r in by["intrusions"]] == [(A, 12, 1, 1), (B, 2, 0, 0), (A, 6, 0, 0)]
    # leading and trailing short runs join the contig's only block
    assert [(r["hap"], r["n_hap"], r["n_switch"], r["n_switch_runs"]) for r in by["leading and trailing"]] == [(A, 6, 2, 2)]
    # A long, B short, A short, B long, A long: the short runs stay with the first block
    assert [(r["hap"], r["n_hap"], r["n_switch"], r["n_switch_runs"]) for r in by["between long runs"]] == [(A, 7, 1, 1), (B, 6, 0, 0), (A, 6, 0, 0)]
    # S = 0: every run is long, a block per run
    got0 = pr.device_records(m.phase_from_planes_host(pr.planes_of(mk, lens), lens, K, 0, 5000))
    assert sum(r["contig"] == names.index("alternating") for r in got0) == 200
    assert all(r["n_switch"] == 0 and r["n_switch_runs"] == 0 for r in got0)
    # a run continued across 3 empty tiles is one run; the same marker count comes out whatever the grid point
    c = names.index("empty tiles")
    e = [r for r in got0 if r["contig"] == c]
    assert [(r["hap"], r["start"], r["end"], r["n_hap"]) for r in e] == [(A, 100, 4 * 4096 + 6, 3), (B, 4 * 4096 + 100, 4 * 4096 + 101, 1),
                                                                        (A, 8 * 4096 + 50, 10 * 4096, 2)]


def test_span_is_exactly_the_range():
    m = _mfx()
    S, R = 3, 64
    names, lens, mk = world(S, R)
    got = pr.device_records(m.phase_from_planes_host(pr.planes_of(mk, lens), lens, K, S, R))
    c = names.index("spans")
    # the intrusion of S markers spanning R bases stays inside, the one spanning R + 1 opens a block
    assert [(r["hap"], r["n_hap"], r["n_switch"]) for r in got if r["contig"] == c] == [(A, 16, 3), (B, 3, 0), (A, 8, 0)]


def test_host_planes_refusals():
    m = _mfx()
    lens = (100,)
    planes = np.zeros((2, 64), dtype=np.uint64)
    assert len(m.phase_from_planes_host(planes, lens, K)) == 0
    planes[1, 1] = np.uint64(1) << np.uint64(36)              # position 100: beyond the contig's 100 positions
    with pytest.raises(m.MfxError) as e:
        m.phase_from_planes_host(planes, lens, K)
    assert e.value.code == -1 and "beyond the 100 positions of contig 0" in str(e.value)
    planes[1, 1] = np.uint64(1) << np.uint64(35)              # position 99: the last one
    assert pr.device_records(m.phase_from_planes_host(planes, lens, K))[0]["start"] == 99
    planes[0, 1] = planes[1, 1]                               # in both planes: shared, no marker
    with pytest.raises(m.MfxError) as e:
        m.phase_from_planes_host(planes, lens, K)
    assert "in both planes" in str(e.value)
    with pytest.raises(m.MfxError):
        m.phase_from_planes_host(np.zeros(5, dtype=np.uint64), lens, K)
    with pytest.raises(m.MfxError):
        m.phase_from_planes_host(np.zeros((2, 64), dtype=np.uint64), lens, 65)
    assert len(m.phase_from_planes_host(np.zeros(0, dtype=np.uint64), (), K)) == 0


def test_api_refusals_without_a_device():
    m = _mfx()
    L = m.load_library()
    from merfin_amd.binding import _PhaseOpts
    o = _PhaseOpts(100, 20000)
    h = C.c_void_p(None)
    assert L.mfx_phase_run(None, None, C.byref(o), C.byref(h)) == -1
    assert b"mfx_phase_run: null argument" in L.mfx_last_error() and not h.value
    assert L.mfx_phase_count(None) == 0
    assert L.mfx_phase_copy(None, None, 0) == -1 and b"mfx_phase_copy" in L.mfx_last_error()
    assert L.mfx_phase_contig_counts(None, None, 0) == -1 and b"mfx_phase_contig_counts" in L.mfx_last_error()
    assert L.mfx_phase_write(None, 0, None, None, None, 21, C.byref(o), b"x") == -1 and b"mfx_phase_write: null argument" in L.mfx_last_error()
    L.mfx_phase_free(None)
    n = C.c_uint64(0)
    assert L.mfx_phase_from_planes_host(None, None, 0, 21, None, None, 0, C.byref(n)) == -1
    assert b"mfx_phase_from_planes_host: null argument" in L.mfx_last_error()
    with pytest.raises(m.MfxError):
        m.binding._phase_opts(-1, 1)
    m.binding._phase_opts(2**64 - 1, 0)                       # any switches and any range are valid


def test_formatters_on_known_records():
    recs = [{"contig": 0, "hap": A, "start": 10, "end": 101, "n_hap": 5, "n_switch": 1, "n_switch_runs": 1},
            {"contig": 0, "hap": B, "start": 200, "end": 211, "n_hap": 2, "n_switch": 0, "n_switch_runs": 0},
            {"contig": 1, "hap": A, "start": 0, "end": 31, "n_hap": 3, "n_switch": 0, "n_switch_runs": 0}]
    assert pr.format_bed(recs, ["x", "y"], 21) == pr.BED_HEADER + "x\t10\t121\tA\t5\t1\t1\nx\t200\t231\tB\t2\t0\t0\ny\t0\t51\tA\t3\t0\t0\n"
    # spans 111, 31, 51: A holds 111 and 51 (sum 162: the 111 block alone is half), all: 193 (111 alone is 57 %)
    assert pr.format_stats(recs, 21, 100, 20000) == ("#switches\t100\trange\t20000\tk\t21\n" + pr.STATS_HEADER + "A\t2\t162\t51\t81\t111\t111\t9\t1\t0.111111\n" +
                                                    "B\t1\t31\t31\t31\t31\t31\t2\t0\t0.000000\n" + "all\t3\t193\t31\t64\t111\t111\t11\t1\t0.090909\n")
    assert pr.format_stats([], 21, 0, 0).endswith("all\t0\t0\t0\t0\t0\t0\t0\t0\t0.000000\n")
    assert pr.format_counts([(100, 3, 4, 5)], ["c"]) == pr.COUNT_HEADER + "c\t3\t4\t5\t100\n"


def test_phase_host_text_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "phase_sanitize")
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "merfin_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "native", "phase_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches, " in r.stdout and "MISMATCH" not in r.stdout
