"""The refusals of `merfin -merge` (cli/args.h: check_merge_flags, and -op in the parser): every line, each made before a device is
touched.  {T} is the test's tmp_path: {T}/a.mfxk and {T}/b.mfxk exist, {T}/none.mfxk does not."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "merfin_amd", "bin", "merfin")

MERGE = ["-merge", "{T}/a.mfxk", "-merge", "{T}/b.mfxk", "-output", "{T}/o.mfxk"]

CASES = [
    (MERGE + ["-hist"], ["-merge is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...)."]),
    (MERGE + ["-spectrum"], ["-merge is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...)."]),
    (MERGE + ["-count"], ["-merge and -count are two operations: give one of them."]),
    (MERGE + ["-convert", "{T}/a.mfxk"], ["-merge and -convert are two operations: give one of them."]),
    (MERGE + ["-reads", "{T}/r.fa"], ["-merge combines databases: it does not take -reads (count them first: -count)."]),
    (MERGE + ["-readmers", "{T}/a.mfxk"], ["-merge takes its databases as -merge <file>: it does not take -readmers."]),
    (MERGE + ["-seqmers", "{T}/a.mfxk"], ["-merge takes its databases as -merge <file>: it does not take -seqmers."]),
    (MERGE + ["-sequence", "{T}/r.fa"], ["-merge evaluates nothing: it does not take -sequence."]),
    (MERGE + ["-vcf", "x.vcf"], ["-merge does not take -vcf (the variant modes do)."]),
    (MERGE + ["-peak", "12"], ["-merge evaluates nothing: it does not take -peak."]),
    (MERGE + ["-peak", "auto"], ["-merge evaluates nothing: it does not take -peak."]),
    (MERGE + ["-sharded"], ["-merge does not take -sharded: the windows it merges live on one device."]),
    (MERGE + ["-index", "{T}/i.idx"], ["-merge does not take -index: it writes a database, not a table image."]),
    (MERGE + ["-placed"], ["-merge writes k-mer-sorted databases: it does not take -placed (convert the result: -convert -placed)."]),
    (MERGE + ["-passes", "3"], ["-passes divides the work of -count: -merge does not take it (MFX_MERGE_RANGE sizes its windows)."]),
    (MERGE + ["-devices", "0-1"], ["-merge runs on one device (-device d, or -devices naming one)."]),
    (MERGE[:-2], ["-merge writes a k-mer database: give -output <file>."]),
    (MERGE + ["-op", "difference"], ["Invalid -op 'difference': the operations of -merge are sum, max, min and intersect."]),
    (MERGE + ["-op"], ["Invalid -op '': the operations of -merge are sum, max, min and intersect."]),
    (MERGE + ["-merge", "{T}/none.mfxk"], ["Cannot read the -merge database '{T}/none.mfxk'."]),
    (["-merge", "{T}/a.mfxk", "-output", "{T}/o.mfxk"] + ["-merge", "{T}/b.mfxk"] * 64, ["-merge takes 1 to 64 databases (here 65): merge them in groups."]),
    # -op without -merge, whatever else the command line is
    (["-op", "max"], ["-op names the operation of -merge: it has no meaning without -merge."]),
    (["-hist", "-sequence", "a", "-output", "o", "-readmers", "r", "-peak", "3", "-op", "sum"], ["-op names the operation of -merge: it has no meaning without -merge."]),
    (["-count", "-reads", "{T}/r.fa", "-k", "21", "-output", "{T}/o.mfxk", "-op", "min"], ["-op names the operation of -merge: it has no meaning without -merge."]),
    # several at once, in the order of the checks
    (["-merge", "{T}/none.mfxk", "-dump", "-count", "-op", "x"],
     ["Invalid -op 'x': the operations of -merge are sum, max, min and intersect.",
      "-merge is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).",
      "-merge and -count are two operations: give one of them.", "-merge writes a k-mer database: give -output <file>.",
      "Cannot read the -merge database '{T}/none.mfxk'."]),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_merge_refusal(tmp_path, case):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    for name in ("a.mfxk", "b.mfxk", "r.fa"):
        (tmp_path / name).write_text(">r0\nACGTACGTACGTACGTACGTACGTACGT\n")      # (refused before a file is opened)
    argv, lines = CASES[case]
    r = subprocess.run([EXE] + [a.replace("{T}", str(tmp_path)) for a in argv], capture_output=True, text=True)
    assert r.returncode == 1, r.stderr
    assert r.stderr.startswith("usage: ")
    # the usage text, the entries of -merge behind it, then exactly the lines of this command line
    head, sep, tail = r.stderr.partition("  Merging k-mer databases (an operation of its own, like -count and -convert):\n")
    assert sep, r.stderr
    entries, _, mine = tail.partition("\n\n")
    assert "-merge db " in entries and "-op o " in entries and "-min / -max ARE applied, to the combined count" in entries
    assert mine.splitlines() == [l.replace("{T}", str(tmp_path)) for l in lines], r.stderr
    assert "HIP device" not in mine                                # refused before a device is asked for
    assert not os.path.exists(str(tmp_path / "o.mfxk")) and not os.path.exists(str(tmp_path / "o.mfxk.blocks"))


def test_usage_without_merge_is_unchanged(tmp_path):
    """a command line that names neither -merge nor -op gets the usage text as it was"""
    r = subprocess.run([EXE, "-bogus"], capture_output=True, text=True)
    assert r.returncode == 1 and "Merging k-mer databases" not in r.stderr and "-merge" not in r.stderr
