"""`merfin -count -reads f1 [-reads f2 ...] -k K -output reads.mfxk`: every flag check fails with return code 1 and its own sentence before
any device is touched (runs on a host without a GPU), and nothing is written; the counting, the table that grows and the database are
checked on the GPU (tests/test_gpu_count.py, tests/test_gpu_cli_count.py)."""
import os

import pytest

from tests.test_cli import EXE, run


@pytest.fixture()
def reads(tmp_path):
    p = tmp_path / "reads.fasta"
    p.write_bytes(b">r0\nACGTACGTTTGACCAGTTACGGATCAGGACTTTACGAC\n")
    return str(p)


def _refused(args, msg, out=None):
    r = run(args)
    assert r.returncode == 1 and msg in r.stderr, (args, r.stderr[-900:])
    assert "usage:" in r.stderr and "ERROR: HIP device" not in r.stderr and "-- Counting" not in r.stderr       # no device was opened
    if out is not None:
        assert not os.path.exists(out)
    return r


def test_count_flag_validation(reads, tmp_path):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    out = str(tmp_path / "reads.mfxk")
    ok = ["-count", "-reads", reads, "-k", "21", "-output", out]
    _refused(["-count", "-k", "21", "-output", out], "-count needs the reads it counts: give -reads <file> (repeatable).\n", out)
    _refused(["-count", "-reads", reads, "-output", out], "-count needs -k: no database gives it.\n", out)
    _refused(["-count", "-reads", reads, "-k", "21"], "-count writes a k-mer database: give -output <file>.\n")
    for k in (32, 33, 64):
        _refused(["-count", "-reads", reads, "-k", str(k), "-output", out],
                 "-count holds k <= 31 (here k = %d): count larger k-mers with `meryl count` and give the database as -readmers.\n" % k, out)
    _refused(ok + ["-readmers", "reads.meryl"], "-count makes the read database: it does not take -readmers.\n", out)
    _refused(ok + ["-seqmers", "asm.meryl"], "-count counts reads: it does not take -seqmers.\n", out)
    _refused(ok + ["-sequence", "asm.fasta"], "-count counts reads: it does not take -sequence.\n", out)
    _refused(ok + ["-vcf", "calls.vcf"], "-count does not take -vcf (the variant modes do).\n", out)
    _refused(ok + ["-peak", "26"], "-count evaluates nothing: it does not take -peak.\n", out)
    _refused(ok + ["-peak", "auto"], "-count evaluates nothing: it does not take -peak.\n", out)
    _refused(ok + ["-sharded"], "-count does not take -sharded: the table it counts into lives on one device.\n", out)
    _refused(ok + ["-index", "img"], "-count does not take -index: it writes a database, not a table image.\n", out)
    _refused(ok + ["-devices", "0,1"], "-count runs on one device (-device d, or -devices naming one).\n", out)
    for mode in ("-hist", "-dump", "-completeness", "-track", "-spectrum", "-filter", "-polish", "-better", "-strict", "-loose"):
        _refused(ok + [mode], "-count is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).\n", out)
    _refused(ok + ["-convert", "db.txt"], "-count and -convert are two operations: give one of them.\n", out)
    _refused(["-count", "-reads", str(tmp_path / "missing.fastq"), "-k", "21", "-output", out],
             "Cannot read the -reads file '%s'.\n" % str(tmp_path / "missing.fastq"), out)
    _refused(ok + ["-bogus"], "Unknown option '-bogus'.\n", out)


def test_each_refusal_comes_alone(reads, tmp_path):
    """one mistake, one sentence: the checks of a report (-sequence, -peak, -readmers missing) do not speak for -count"""
    out = str(tmp_path / "reads.mfxk")
    r = _refused(["-count", "-reads", reads, "-k", "33", "-output", out], "-count holds k <= 31 (here k = 33)", out)
    errs = r.stderr.split("[-comb N (15)] [-nosplit] [-debug -> <output>.00.debug.gz]\n\n", 1)[1]
    assert errs.count("\n") == 1, errs
    for msg in ("No input sequences", "No haploid peak", "No read meryl database", "No report type", "-reads needs -k", "-convert rewrites"):
        assert msg not in r.stderr


def test_a_clean_line_passes_validation(reads, tmp_path):
    """-min / -max / -memory / -device / -threads are taken; such a line stops at the device that is not there or runs"""
    out = str(tmp_path / "reads.mfxk")
    r = run(["-count", "-reads", reads, "-reads", reads, "-k", "21", "-output", out, "-min", "2", "-max", "900", "-memory", "4", "-device", "0",
             "-threads", "4", "-devices", "0"])
    assert "usage:" not in r.stderr, r.stderr[-600:]
    assert r.returncode == 0 or "ERROR: HIP device 0 not available" in r.stderr


def test_usage_names_count():
    r = run([])
    assert r.returncode == 1
    assert "    -count            no report: count every k-mer of the -reads files on the GPU" in r.stderr
    # the lines that were there stay
    assert "    -convert db       no report: rewrite the k-mer database <db>" in r.stderr
    assert "No report type (-filter, -polish, -hist, -dump, -completeness) supplied." in r.stderr
