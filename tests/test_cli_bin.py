"""`merfin -bin -reads f -hapmers A -hapmers B -output stem [-ratio r] [-minhits m] [-split]`: every flag check fails with return code 1
and its own message before any device is touched (runs on a host without a GPU); the usage names -bin only for a command line that
names one of its flags, behind the usage text that was there, which stays byte for byte.  The counts and the files are checked on the
GPU (tests/test_gpu_bin.py, tests/test_gpu_cli_bin.py)."""
import os

import numpy as np
import pytest

from tests.test_cli import EXE, run

ENTRY = "  Trio binning (an operation of its own: no -sequence, no -readmers, no -peak):\n"
HIST = ["-hist", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26", "-output", "out"]


def _db(path, k, kmers):
    import merfin_amd as m
    kmers = np.array(sorted(kmers), dtype=np.uint64)
    m.db_write_flat(str(path), k, kmers, np.ones(len(kmers), dtype=np.uint32))
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """two 21-mer databases and a 15-mer one (host only: the writer needs no device), and a read file"""
    d = tmp_path_factory.mktemp("bin")
    reads = d / "reads.fa"
    reads.write_text(">r1\nACGTACGTACGTACGTACGTACGTACGT\n")
    return {"A": _db(d / "a.mfxk", 21, [5, 9, 77]), "B": _db(d / "b.mfxk", 21, [6, 8]), "K15": _db(d / "c.mfxk", 15, [3, 4]), "R": str(reads),
            "dir": d}


def _base(f, *extra, a="A", b="B"):
    return ["-bin", "-reads", f["R"], "-hapmers", f[a], "-hapmers", f[b], "-output", "out"] + list(extra)


def _cases(f):
    A, B, R = f["A"], f["B"], f["R"]
    gone = str(f["dir"] / "gone.fq")
    cases = [
        (["-bin", "-reads", R, "-output", "out"], ["-bin takes exactly two -hapmers databases, haplotype A then B (here 0).\n"]),
        (["-bin", "-reads", R, "-hapmers", A, "-output", "out"], ["-bin takes exactly two -hapmers databases, haplotype A then B (here 1).\n"]),
        (_base(f, "-hapmers", A), ["-bin takes exactly two -hapmers databases, haplotype A then B (here 3).\n"]),
        (HIST + ["-ratio", "2"], ["-ratio sets the class rule of -bin; it has no meaning without -bin.\n"]),
        (HIST + ["-minhits", "2"], ["-minhits sets the class rule of -bin; it has no meaning without -bin.\n"]),
        (HIST + ["-split"], ["-split writes the reads of -bin per class; it has no meaning without -bin.\n"]),
        (["-bin", "-hapmers", A, "-hapmers", B, "-output", "out"], ["-bin needs the reads it sorts: give -reads <file> (repeatable).\n"]),
        (_base(f, "-reads", gone), ["Cannot read the -reads file '%s'.\n" % gone]),
        (_base(f, "-sequence", "asm.fa"), ["-bin sorts reads, it evaluates no assembly: it does not take -sequence (-phase does).\n"]),
        (_base(f, "-readmers", "r.meryl"), ["-bin takes its k-mers as -hapmers <file>: it does not take -readmers.\n"]),
        (_base(f, "-seqmers", "s.meryl"), ["-bin takes its k-mers as -hapmers <file>: it does not take -seqmers.\n"]),
        (_base(f, "-peak", "26"), ["-bin evaluates no K*: it does not take -peak.\n"]),
        (_base(f, "-peak", "auto"), ["-bin evaluates no K*: it does not take -peak.\n"]),
        (_base(f, "-prob", "table.txt"), ["-bin evaluates no K*: it does not take -prob.\n"]),
        (_base(f, "-vcf", "calls.vcf"), ["-bin does not take -vcf (the variant modes do).\n"]),
        (_base(f, "-sharded", "-devices", "0,1"), ["-bin does not take -sharded: a read's counts need both sets' whole membership on one device.\n",
                                                   "-bin runs on one device (-device d, or -devices naming one).\n"]),
        (_base(f, "-devices", "0,1"), ["-bin runs on one device (-device d, or -devices naming one).\n"]),
        (_base(f, "-index", "i"), ["-bin does not take -index: its table holds the two hap-mer sets, not a run's counts.\n"]),
        (_base(f, "-join"), ["-join is a way to run -completeness and -spectrum: -bin does not take it.\n"]),
        (_base(f, "-hist"), ["-bin is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).\n"]),
        (_base(f, "-regions"), ["-bin is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).\n"]),
        (_base(f, "-merge", A), ["-bin, -phase, -count, -convert and -merge are separate operations: give one of them.\n"]),
        (_base(f, "-count"), ["-bin, -phase, -count, -convert and -merge are separate operations: give one of them.\n"]),
        (_base(f, "-convert", A), ["-bin, -phase, -count, -convert and -merge are separate operations: give one of them.\n"]),
        (_base(f, "-phase"), ["-bin, -phase, -count, -convert and -merge are separate operations: give one of them.\n"]),
        (_base(f, "-switches", "3"), ["-switches and -range bound the switch errors of -phase: -bin does not take them.\n"]),
        (_base(f, a="A", b="A"), ["-bin needs two different hap-mer sets: both -hapmers name '%s'.\n" % A]),
        (_base(f, b="K15"), ["The two -hapmers databases hold different k-mers: 21-mers and 15-mers.\n"]),
        (_base(f, "-k", "15"), ["-k 15 disagrees with -hapmers, which hold 21-mers.\n"]),
        (["-bin", "-reads", R, "-hapmers", A, "-hapmers", B], ["No output (-output) supplied.\n"]),
    ]
    for bad in ("0.999", "0", "-2", "1.0005", "2.", ".5", "x", "1e3", "", " 2", "2,5", "4000001"):
        cases.append((_base(f, "-ratio", bad), ["Invalid -ratio '%s': the ratio of -bin is a decimal of at most three places, 1 to 4000000.\n" % bad]))
    for bad in ("-1", "1.5", "x", "", "4294967296"):
        cases.append((_base(f, "-minhits", bad), ["Invalid -minhits '%s': -minhits is a number of k-mers, an integer from 0 to 4294967295.\n" % bad]))
    return cases


N_CASES = 30 + 12 + 5


@pytest.mark.parametrize("case", range(N_CASES))
def test_bin_refusal(case, files):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    cases = _cases(files)
    assert len(cases) == N_CASES
    argv, lines = cases[case]
    r = run(argv)
    assert r.returncode == 1, r.stderr
    assert r.stderr.startswith("usage: ")
    head, sep, tail = r.stderr.partition(ENTRY)
    assert sep, r.stderr                                       # the command line names a flag of -bin: its entries follow the usage
    _, _, mine = tail.partition("\n\n")
    assert mine.splitlines(keepends=True) == lines, r.stderr  # these lines and no other
    assert "ERROR: HIP device" not in r.stderr                # no device was opened


def test_a_missing_hapmers_database_is_named(files, tmp_path):
    gone = str(tmp_path / "gone.mfxk")
    r = run(["-bin", "-reads", files["R"], "-hapmers", gone, "-hapmers", files["B"], "-output", "out"])
    assert r.returncode == 1 and ENTRY in r.stderr
    assert any(l.startswith("Cannot open the -hapmers database '%s': " % gone) for l in r.stderr.splitlines()), r.stderr
    assert "ERROR: HIP device" not in r.stderr


def test_wide_hapmers_are_refused(files, tmp_path):
    """k = 33: two databases in the `meryl print` text form, one 33-mer each"""
    a, b = tmp_path / "a33.txt", tmp_path / "b33.txt"
    a.write_text("ACGTACGTACGTACGTACGTACGTACGTACGTA\t3\n")
    b.write_text("ACGTACGTACGTACGTACGTACGTACGTACGTC\t2\n")
    r = run(["-bin", "-reads", files["R"], "-hapmers", str(a), "-hapmers", str(b), "-output", "out"])
    assert r.returncode == 1 and r.stderr.startswith("usage: ") and "ERROR: HIP device" not in r.stderr
    assert r.stderr.endswith("\n\n-bin holds k <= 31 (here k = 33): hap-mer databases of larger k-mers are not binned.\n"), r.stderr


def test_a_clean_bin_line_trips_no_check(files):
    """each check has its own message: a clean line gets past all of them and stops at the device that is not there (on a machine
    that has one it runs)"""
    out = str(files["dir"] / "clean")
    r = run(["-bin", "-reads", files["R"], "-reads", files["R"], "-hapmers", files["A"], "-hapmers", files["B"], "-output", out, "-ratio", "2.125", "-minhits", "0", "-split",
             "-devices", "0", "-min", "1", "-k", "21"])
    assert not r.stderr.startswith("usage: ") and ENTRY not in r.stderr, r.stderr
    assert (r.returncode == 1 and "ERROR: HIP device 0 not available" in r.stderr) or (r.returncode == 0 and "ratio 2.125, at least 0 hits" in r.stderr), r.stderr


def test_usage_names_bin_only_when_asked_for():
    plain = run([])
    assert plain.returncode == 1 and "-bin" not in plain.stderr and "-ratio" not in plain.stderr and "-minhits" not in plain.stderr and "-split" not in plain.stderr
    asked = run(["-bin"])
    assert asked.returncode == 1
    head, sep, tail = asked.stderr.partition(ENTRY)
    assert sep and "    -bin " in tail and "    -hapmers db " in tail and "    -ratio r " in tail and "    -minhits m " in tail and "    -split " in tail
    assert "<output>.bin.tsv" in tail and "<output>.bin.stats" in tail and "<output>.hapA.fasta" in tail and "<output>.unknown.fasta" in tail
    assert "not validated against Canu" in tail and "drops the qualities" in tail
    # the usage text that was there is the same text, byte for byte, and comes first
    usage_plain = plain.stderr[:plain.stderr.index("No input sequences")]
    assert head == usage_plain
    # the other operations' entries stay where they were, and theirs do not name -bin
    assert "-bin" not in run(["-merge", "a", "-bogus"]).stderr and "-bin" not in run(["-regions"]).stderr and "-bin" not in run(["-phase"]).stderr
    # -hapmers without -bin is still -phase's flag
    r = run(HIST + ["-hapmers", "x"])
    assert r.stderr.endswith("\n\n-hapmers names a hap-mer database of -phase; it has no meaning without -phase.\n") and ENTRY not in r.stderr
