"""`merfin -count -passes P|auto` end to end on the GPU: under a -memory that refuses the table of one pass the run completes in passes
over key ranges, and the database is byte for byte the one of the unlimited single pass and of the oracle's counts -- from the read store
and from the files, with a pilot (-passes 3) and without (-passes auto)."""
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import synth_reads as sr
from tests.test_cli import _write_fasta, run
from tests.test_gpu_cli_count import _write_fastq

pytestmark = pytest.mark.gpu

BATCH = 4096                                                   # MFX_COUNT_BATCH: small batches reach growth on a small read set
SLOTS_LINE, START_LINES, LINE_BYTES = 8, 1024, 128


# ---- the two rules of csrc/mfx_grow.h, restated
def grow_fits(distinct, pending, B, slots):
    return 10 * (distinct + pending + B) <= 7 * slots


def grow_lines(distinct, B, nlines):
    mult = 2
    while 20 * (distinct + B) > 7 * nlines * mult * SLOTS_LINE:
        mult *= 2
    return nlines * mult


def _tables(D):
    """the tables a counter with batches of BATCH positions goes through from START_LINES lines while it claims D k-mers: a launch needs
    distinct + pending + B <= 0.7 x slots, so the table that ends with D k-mers has D <= 0.7 x slots, and it grows from a table when the
    known count d has d + B > 0.7 x slots -- with d at most what that table may hold.  Returns the list of line counts."""
    lines = [START_LINES]
    while 10 * D > 7 * lines[-1] * SLOTS_LINE:
        d = 7 * lines[-1] * SLOTS_LINE // 10                      # the most the table held when the bound failed
        assert not grow_fits(d, 0, BATCH, lines[-1] * SLOTS_LINE)
        lines.append(grow_lines(d, BATCH, lines[-1]))
    return lines


def _memory_that_refuses_one_pass(rk, k):
    """-memory in GB: the growth the whole range needs is refused, the growths of each half are not"""
    bins = np.bincount((rk >> np.uint64(2 * k - 12)).astype(np.int64), minlength=4096)
    c = np.cumsum(bins)
    half = min(max(int(c[i]), int(c[-1] - c[i])) for i in range(4095))         # the larger half of the best cut at a bin boundary
    whole_t, half_t = _tables(len(rk)), _tables(half)
    assert half + BATCH <= 7 * half_t[-1] * SLOTS_LINE // 10                   # a half never asks its last table to grow, whatever the batches hold
    assert len(whole_t) > len(half_t) and whole_t[:len(half_t)] == half_t
    fits = max((a + b) * LINE_BYTES for a, b in zip(half_t, half_t[1:]))       # both tables are held while the entries move
    refused = (whole_t[len(half_t) - 1] + whole_t[len(half_t)]) * LINE_BYTES
    assert fits < refused
    limit = (fits + refused) // 2
    return limit / 1e9


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _files(tmp_path, reads):
    half = len(reads) // 2
    fq, fa = str(tmp_path / "a.fastq"), str(tmp_path / "b.fasta.gz")
    _write_fastq(fq, [x for x in reads[:half] if x])
    _write_fasta(fa, reads[half:], gz=True)
    return ["-reads", fq, "-reads", fa]


def _count(tmp_path, name, k, files, extra, env=None, memory=None):
    import os
    out = str(tmp_path / name)
    e = dict(os.environ, MFX_COUNT_BATCH=str(BATCH))
    e.update(env or {})
    args = ["-count"] + files + ["-k", str(k), "-output", out] + extra + (["-memory", "%.9f" % memory] if memory else [])
    return out, run(args, env=e)


def _passes(stderr):
    return re.findall(r"^-- Pass (\d+): bins \[(\d+), (\d+)\) of 4096: (\d+) k-mers counted, (\d+) distinct, table \d+\.\d{3} GB, \d+\.\d\d s, (from memory|from the files)\.$",
                      stderr, re.M)


def _check_passes(r, rk, rv, source=None):
    """the pass lines are a partition of the bins in ascending order and add up; returns (passes, refused)"""
    ps = _passes(r.stderr)
    assert ps and [int(p[0]) for p in ps] == list(range(1, len(ps) + 1))
    assert int(ps[0][1]) == 0 and int(ps[-1][2]) == 4096 and all(int(a[2]) == int(b[1]) for a, b in zip(ps, ps[1:]))
    assert sum(int(p[3]) for p in ps) == int(rv.sum()) and sum(int(p[4]) for p in ps) == len(rk)
    if source:
        assert all(p[5] == source for p in ps), r.stderr
    mm = re.search(r"-- Counted the \d+-mers of \d+ reads \(\d+ bases\): %d k-mers, %d distinct; the table grew \d+ times? to \d+\.\d{3} GB in (\d+) pass(?:es)? \((\d+) refused and split\)\.\n"
                   % (int(rv.sum()), len(rk)), r.stderr)
    assert mm and int(mm.group(1)) == len(ps), r.stderr
    assert len(re.findall(r"^-- Bins \[\d+, \d+\) of 4096: refused, ", r.stderr, re.M)) == int(mm.group(2))
    return len(ps), int(mm.group(2))


def test_passes_under_a_memory_that_refuses_one_pass(tmp_path):
    m = _mfx()
    import os
    k = 21
    asm, reads = sr.reads_world(k, 1721, sizes=(12000, 4096, 500), n_reads=1000)
    rk, rv = po.count_kmers(k, reads)
    files = _files(tmp_path, reads)
    want = str(tmp_path / "want.mfxk")
    m.db_write_flat(want, k, rk, rv)
    want_bytes = open(want, "rb").read()
    gb = _memory_that_refuses_one_pass(rk, k)
    # one pass without a limit: the database
    one, r = _count(tmp_path, "one.mfxk", k, files, [])
    assert r.returncode == 0 and open(one, "rb").read() == want_bytes, r.stderr
    # one pass under the limit: refused with the library's sentence and the hint, nothing written
    out, r = _count(tmp_path, "refused.mfxk", k, files, [], memory=gb)
    assert r.returncode == 1 and not os.path.exists(out), r.stderr
    assert "ERROR: counting -reads: " in r.stderr and "the k-mer table cannot grow from" in r.stderr and "both tables are held while the entries move" in r.stderr
    assert r.stderr.rstrip().endswith("-- Hint: -passes auto counts the k-mers in passes over key ranges, each in a table of its own that fits -memory and the device.")
    # -passes auto under it: at least one range refused and split, the same bytes
    out, r = _count(tmp_path, "auto.mfxk", k, files, ["-passes", "auto"], memory=gb)
    assert r.returncode == 0, r.stderr
    n_pass, n_refused = _check_passes(r, rk, rv, "from memory")                 # by default every pass runs from the store
    assert n_refused >= 1 and n_pass >= 2
    assert open(out, "rb").read() == want_bytes
    # the same without a store: every pass reads the files
    out, r = _count(tmp_path, "auto_files.mfxk", k, files, ["-passes", "auto"], env={"MFX_COUNT_STORE_GB": "0"}, memory=gb)
    assert r.returncode == 0, r.stderr
    n_pass, n_refused = _check_passes(r, rk, rv, "from the files")
    assert n_refused >= 1 and n_pass >= 2
    assert open(out, "rb").read() == want_bytes
    # a store that fills up: dropped, every pass reads the files
    out, r = _count(tmp_path, "auto_full.mfxk", k, files, ["-passes", "2"], env={"MFX_COUNT_STORE_GB": "0.00005"})
    assert r.returncode == 0 and "-- The read store is full at 0.000 GB (MFX_COUNT_STORE_GB): every pass reads the files.\n" in r.stderr, r.stderr
    assert _check_passes(r, rk, rv, "from the files") == (2, 0)
    assert open(out, "rb").read() == want_bytes
    # -passes 3 without a limit: the pilot's three ranges, nothing refused; -passes 1: one pass
    out, r = _count(tmp_path, "three.mfxk", k, files, ["-passes", "3"])
    assert r.returncode == 0, r.stderr
    assert _check_passes(r, rk, rv, "from memory") == (3, 0)
    assert open(out, "rb").read() == want_bytes
    out1, r = _count(tmp_path, "p1.mfxk", k, files, ["-passes", "1"])
    assert r.returncode == 0 and _check_passes(r, rk, rv, "from memory") == (1, 0), r.stderr
    assert open(out1, "rb").read() == want_bytes
    # -completeness from the file of three passes is -completeness from the file of one
    fa = str(tmp_path / "asm.fasta")
    _write_fasta(fa, asm)
    a = run(["-completeness", "-sequence", fa, "-readmers", out, "-peak", "9"])
    b = run(["-completeness", "-sequence", fa, "-readmers", one, "-peak", "9"])
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    lines = lambda s: [l for l in s.splitlines() if l.startswith(("TOTAL", "COMPLETENESS", "thread "))]
    assert a.stdout == b.stdout and lines(a.stderr) == lines(b.stderr) and len(lines(a.stderr)) == 64 + 3


def test_even_k_with_palindromes_in_passes(tmp_path):
    """k = 22: a k-mer that is its own reverse complement is counted once per occurrence in whichever pass holds it"""
    m = _mfx()
    k = 22
    asm, reads = sr.reads_world(k, 1722, sizes=(12000, 4096, 500), n_reads=1000)
    pal = b"ACGTTGCAAGCTTGCAACGT"
    reads = reads + [b"A" + pal + b"T", b"AATTCCGGAACCGGTTCCGGAATT" * 3, b"G" + pal + b"C"]
    rk, rv = po.count_kmers(k, reads)
    files = _files(tmp_path, reads)
    want = str(tmp_path / "want.mfxk")
    m.db_write_flat(want, k, rk, rv)
    gb = _memory_that_refuses_one_pass(rk, k)
    out, r = _count(tmp_path, "auto.mfxk", k, files, ["-passes", "auto"], memory=gb)
    assert r.returncode == 0, r.stderr
    n_pass, n_refused = _check_passes(r, rk, rv, "from memory")
    assert n_refused >= 1 and n_pass >= 2
    assert open(out, "rb").read() == open(want, "rb").read()
    out, r = _count(tmp_path, "four.mfxk", k, files, ["-passes", "4"], env={"MFX_COUNT_STORE_GB": "0"})
    assert r.returncode == 0 and _check_passes(r, rk, rv, "from the files") == (4, 0), r.stderr
    assert open(out, "rb").read() == open(want, "rb").read()
