"""`merfin -phase -hapmers A -hapmers B [-switches S] [-range R]`: every flag check fails with return code 1 and its own message before
any device is touched (runs on a host without a GPU); the usage names -phase only for a command line that names one of its flags,
behind the usage text that was there, which stays byte for byte.  The records and the files are checked on the GPU
(tests/test_gpu_phase.py, tests/test_gpu_cli_phase.py)."""
import os

import numpy as np
import pytest

from tests.test_cli import EXE, run

ENTRY = "  Trio phasing (an operation of its own: no -readmers, no -peak):\n"


def _db(path, k, kmers):
    import merfin_amd as m
    kmers = np.array(sorted(kmers), dtype=np.uint64)
    m.db_write_flat(str(path), k, kmers, np.ones(len(kmers), dtype=np.uint32))
    return str(path)


@pytest.fixture(scope="module")
def dbs(tmp_path_factory):
    """two 21-mer databases and a 15-mer one (host only: the writer needs no device)"""
    d = tmp_path_factory.mktemp("hapmers")
    return {"A": _db(d / "a.mfxk", 21, [5, 9, 77]), "B": _db(d / "b.mfxk", 21, [6, 8]), "K15": _db(d / "c.mfxk", 15, [3, 4])}


def _base(dbs, *extra, a="A", b="B"):
    return ["-phase", "-sequence", "asm.fa", "-hapmers", dbs[a], "-hapmers", dbs[b], "-output", "out"] + list(extra)


HIST = ["-hist", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26", "-output", "out"]


def _cases(dbs):
    A, B = dbs["A"], dbs["B"]
    cases = [
        (["-phase", "-sequence", "asm.fa", "-output", "out"], ["-phase takes exactly two -hapmers databases, haplotype A then B (here 0).\n"]),
        (["-phase", "-sequence", "asm.fa", "-hapmers", A, "-output", "out"], ["-phase takes exactly two -hapmers databases, haplotype A then B (here 1).\n"]),
        (_base(dbs, "-hapmers", A), ["-phase takes exactly two -hapmers databases, haplotype A then B (here 3).\n"]),
        (HIST + ["-hapmers", A], ["-hapmers names a hap-mer database of -phase; it has no meaning without -phase.\n"]),
        (HIST + ["-switches", "5"], ["-switches bounds the switch errors of -phase; it has no meaning without -phase.\n"]),
        (HIST + ["-range", "5"], ["-range bounds the switch errors of -phase; it has no meaning without -phase.\n"]),
        (_base(dbs, "-readmers", "r.meryl"), ["-phase takes its k-mers as -hapmers <file>: it does not take -readmers.\n"]),
        (_base(dbs, "-seqmers", "s.meryl"), ["-phase does not count the assembly's k-mers: it does not take -seqmers.\n"]),
        (_base(dbs, "-reads", "r.fq", "-k", "21"), ["-phase takes databases of hap-mers: it does not take -reads (count them first: -count).\n"]),
        (_base(dbs, "-peak", "26"), ["-phase evaluates no K*: it does not take -peak.\n"]),
        (_base(dbs, "-peak", "auto"), ["-phase evaluates no K*: it does not take -peak.\n"]),
        (_base(dbs, "-prob", "table.txt"), ["-phase evaluates no K*: it does not take -prob.\n"]),
        (_base(dbs, "-vcf", "calls.vcf"), ["-phase does not take -vcf (the variant modes do).\n"]),
        (_base(dbs, "-sharded", "-devices", "0,1"), ["-phase does not take -sharded: a marker needs both sets' whole membership on one device.\n",
                                                     "-phase runs on one device (-device d, or -devices naming one).\n"]),
        (_base(dbs, "-devices", "0,1"), ["-phase runs on one device (-device d, or -devices naming one).\n"]),
        (_base(dbs, "-index", "i"), ["-phase does not take -index: its table holds the two hap-mer sets, not a run's counts.\n"]),
        (_base(dbs, "-hist"), ["-phase is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).\n"]),
        (_base(dbs, "-merge", A), ["-phase, -count, -convert and -merge are separate operations: give one of them.\n"]),
        (_base(dbs, "-count"), ["-phase, -count, -convert and -merge are separate operations: give one of them.\n"]),
        (_base(dbs, a="A", b="A"), ["-phase needs two different hap-mer sets: both -hapmers name '%s'.\n" % A]),
        (_base(dbs, b="K15"), ["The two -hapmers databases hold different k-mers: 21-mers and 15-mers.\n"]),
        (["-phase", "-hapmers", A, "-hapmers", B, "-output", "out"], ["No input sequences (-sequence) supplied.\n"]),
        (["-phase", "-sequence", "asm.fa", "-hapmers", A, "-hapmers", B], ["No output (-output) supplied.\n"]),
    ]
    for bad in ("-5", "1.5", "x", "10k", "", "+7", " 7", "99999999999999999999999"):
        cases.append((_base(dbs, "-switches", bad), ["Invalid -switches '%s': -switches is a number of markers, an integer of at least 0.\n" % bad]))
        cases.append((_base(dbs, "-range", bad), ["Invalid -range '%s': -range is a number of bases, an integer of at least 0.\n" % bad]))
    return cases


N_CASES = 23 + 16


@pytest.mark.parametrize("case", range(N_CASES))
def test_phase_refusal(case, dbs):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    cases = _cases(dbs)
    assert len(cases) == N_CASES
    argv, lines = cases[case]
    r = run(argv)
    assert r.returncode == 1, r.stderr
    assert r.stderr.startswith("usage: ")
    head, sep, tail = r.stderr.partition(ENTRY)
    assert sep, r.stderr                                       # the command line names a flag of -phase: its entries follow the usage
    _, _, mine = tail.partition("\n\n")
    assert mine.splitlines(keepends=True) == lines, r.stderr  # these lines and no other
    assert "ERROR: HIP device" not in r.stderr                # no device was opened


def test_a_missing_hapmers_database_is_named(dbs, tmp_path):
    gone = str(tmp_path / "gone.mfxk")
    r = run(_base(dbs) [:4] + [gone, "-hapmers", dbs["B"], "-output", "out"])
    assert r.returncode == 1 and ENTRY in r.stderr
    assert any(l.startswith("Cannot open the -hapmers database '%s': " % gone) for l in r.stderr.splitlines()), r.stderr
    assert "ERROR: HIP device" not in r.stderr


def test_a_clean_phase_line_trips_no_check(dbs):
    """each check has its own message: a clean line gets past all of them and stops at the device that is not there (or, on a
    machine that has one, at the sequence file that is not there)"""
    r = run(_base(dbs, "-switches", "0", "-range", "0", "-devices", "0", "-min", "1"))
    assert not r.stderr.startswith("usage: ") and ENTRY not in r.stderr, r.stderr
    assert r.returncode == 1
    assert "ERROR: HIP device 0 not available" in r.stderr or "cannot open 'asm.fa'" in r.stderr, r.stderr


def test_usage_names_phase_only_when_asked_for():
    plain = run([])
    assert plain.returncode == 1 and "-phase" not in plain.stderr and "-hapmers" not in plain.stderr and "-switches" not in plain.stderr
    asked = run(["-phase"])
    assert asked.returncode == 1
    head, sep, tail = asked.stderr.partition(ENTRY)
    assert sep and "    -phase " in tail and "    -hapmers db " in tail and "    -switches S " in tail and "    -range R " in tail
    assert "<output>.phased_block.bed" in tail and "<output>.hapmers.count" in tail and "<output>.phased_block.stats" in tail
    assert "not validated against Merqury" in tail
    # the usage text that was there is the same text, byte for byte, and comes first
    usage_plain = plain.stderr[:plain.stderr.index("No input sequences")]
    assert head == usage_plain
    # the other operations' entries stay where they were
    assert "-phase" not in run(["-merge", "a", "-bogus"]).stderr and "-phase" not in run(["-regions"]).stderr


def test_not_belongs_to_merge(dbs, tmp_path):
    """-not: refused without -merge with its own text; its usage entry is printed only for a command line that names it"""
    r = run(HIST + ["-not", dbs["A"]])
    assert r.returncode == 1 and r.stderr.startswith("usage: ")
    assert r.stderr.endswith("\n\n-not names a database to subtract in -merge: it has no meaning without -merge.\n"), r.stderr
    assert "    -not db           with -merge: the k-mers of this sorted flat database are not written" in r.stderr
    assert "ERROR: HIP device" not in r.stderr
    assert "-not db" not in run(["-merge", "a", "-bogus"]).stderr and "-not db" not in run([]).stderr
    gone = str(tmp_path / "gone.mfxk")
    r = run(["-merge", dbs["A"], "-not", gone, "-output", str(tmp_path / "o.mfxk")])
    assert r.returncode == 1 and r.stderr.endswith("Cannot read the -not database '%s'.\n" % gone), r.stderr
    r = run(["-merge", dbs["A"], "-output", str(tmp_path / "o.mfxk")] + ["-not", dbs["B"]] * 64)
    assert r.returncode == 1 and r.stderr.endswith("-merge and -not take 64 databases at the most (here 1 and 64).\n"), r.stderr
    # -op difference stays refused, with the text that lists four operations
    r = run(["-merge", dbs["A"], "-op", "difference", "-output", str(tmp_path / "o.mfxk")])
    assert r.returncode == 1 and "Invalid -op 'difference': the operations of -merge are sum, max, min and intersect.\n" in r.stderr
