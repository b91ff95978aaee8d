"""`merfin -regions [-kstar t] [-gap g] [-minrun m]`: every flag check fails with return code 1 and its own message before any device
is touched (runs on a host without a GPU); the usage names -regions only for a command line that names one of its flags, behind
the usage text that was there, which stays byte for byte.  The records and the file are checked on the GPU (tests/test_gpu_regions.py,
tests/test_gpu_cli_regions.py)."""
import os

import pytest

from tests.test_cli import EXE, run

ENTRY = "  Intervals instead of windows (a report type, like -track):\n"


def _base(*extra):
    return ["-regions", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26", "-output", "out"] + list(extra)


CASES = [
    (_base("-sharded", "-devices", "0,1"), ["-regions does not take -sharded: a k-mer's class needs its whole counts on one device.\n",
                                            "-regions runs on one device (-device d, or -devices naming one).\n"]),
    (_base("-devices", "0,1"), ["-regions runs on one device (-device d, or -devices naming one).\n"]),
    (_base("-vcf", "calls.vcf"), ["-regions does not take -vcf (the variant modes do).\n"]),
    (_base("-skipMissing"), ["-skipMissing belongs to -dump; -regions writes the missing k-mers as intervals.\n"]),
    (["-hist", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26", "-output", "out", "-kstar", "2"],
     ["-kstar sets the threshold of -regions; it has no meaning without -regions.\n"]),
    (["-track", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26", "-output", "out", "-gap", "5"],
     ["-gap joins the runs of -regions; it has no meaning without -regions.\n"]),
    (["-dump", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26", "-output", "out", "-minrun", "5"],
     ["-minrun drops short regions of -regions; it has no meaning without -regions.\n"]),
    (["-regions", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26"], ["No output (-output) supplied.\n"]),
    (["-regions", "-readmers", "reads.meryl", "-peak", "26", "-output", "out"], ["No input sequences (-sequence) supplied.\n"]),
    (["-regions", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-output", "out"], ["No haploid peak (-peak) supplied.\n"]),
]
for bad in ("0", "-1", "x", "", "inf", "nan", "1e999", "1.5x", " 2"):
    CASES.append((_base("-kstar", bad), ["Invalid -kstar '%s': the threshold of -regions is a finite number above 0.\n" % bad]))
for bad in ("-5", "1.5", "x", "10k", "", "+7", " 7", "99999999999999999999999"):
    CASES.append((_base("-gap", bad), ["Invalid -gap '%s': a gap is a number of positions, an integer of at least 0.\n" % bad]))
    CASES.append((_base("-minrun", bad), ["Invalid -minrun '%s': -minrun is a number of k-mers, an integer of at least 0.\n" % bad]))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_regions_refusal(case):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    argv, lines = CASES[case]
    r = run(argv)
    assert r.returncode == 1, r.stderr
    assert r.stderr.startswith("usage: ")
    head, sep, tail = r.stderr.partition(ENTRY)
    assert sep, r.stderr                                       # the command line names a flag of -regions: its entries follow the usage
    _, _, mine = tail.partition("\n\n")
    assert mine.splitlines(keepends=True) == lines, r.stderr  # these lines and no other
    assert "ERROR: HIP device" not in r.stderr                # no device was opened


def test_a_clean_regions_line_trips_no_check():
    """each check has its own message: a clean line gets past all of them and stops at the database that is not there"""
    r = run(_base("-kstar", "0.5", "-gap", "20", "-minrun", "21", "-devices", "0"))
    assert not r.stderr.startswith("usage: ") and ENTRY not in r.stderr, r.stderr
    for msg in ("-regions does not", "-regions runs", "-skipMissing belongs", "No output", "Invalid -", "-kstar sets", "-gap joins", "-minrun drops"):
        assert not any(l.startswith(msg) for l in r.stderr.splitlines()), r.stderr
    assert r.returncode == 1                                   # (reads.meryl does not exist)


def test_usage_names_regions_only_when_asked_for():
    plain = run([])
    assert plain.returncode == 1 and "-regions" not in plain.stderr and "-kstar" not in plain.stderr and "-minrun" not in plain.stderr
    asked = run(["-regions"])
    assert asked.returncode == 1
    head, sep, tail = asked.stderr.partition(ENTRY)
    assert sep and "    -regions " in tail and "    -kstar t " in tail and "    -gap g " in tail and "    -minrun m " in tail and "<output>.regions.bed" in tail
    # the usage text that was there is the same text, byte for byte, and comes first
    usage_plain = plain.stderr[:plain.stderr.index("No input sequences")]
    assert head == usage_plain
    assert "    -track          K* summarised per window of every contig on the GPU -> <output>.track.tsv, <output>.kstar.bedgraph\n" in head
    assert "    -dump           seqName, seqPos, readK, asmK, K* per k-mer to <output>  [-skipMissing]\n" in head
    # the other operations' entries stay where they were
    assert "-regions" not in run(["-merge", "a", "-bogus"]).stderr
