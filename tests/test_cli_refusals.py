"""The refusals of the `merfin` CLI, pinned: every command line that fails its flag checks ends before a device is touched, with the
same exit code and the same bytes on stderr wherever it runs.  CASES holds, per argv, the exit code and the exact stderr lines with the
usage text collapsed to "<usage>" (its own bytes are pinned once, by USAGE_CRC).  The table was recorded from the binary of the commit
before main() was split into parse, check, build and report steps; `python tests/test_cli_refusals.py` prints it anew from the built binary.

{T} is the test's tmp_path: {T}/r.fa is a -reads file that exists, {T}/none.fa one that does not, {T}/asm.txt a two-line `meryl print`
text of 5-mers for the one check that has to open -seqmers (its k against -k).  Nothing else of the file system is touched."""
import os
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "merfin_amd", "bin", "merfin")
USAGE_END = "                    [-comb N (15)] [-nosplit] [-debug -> <output>.00.debug.gz]\n\n"
USAGE_CRC = 96821944

HIST = ["-hist", "-sequence", "a", "-output", "o", "-readmers", "r", "-peak", "3"]
COUNT = ["-count", "-reads", "{T}/r.fa", "-k", "21", "-output", "{T}/o.mfxk"]
READS = ["-hist", "-sequence", "a", "-output", "o", "-peak", "3", "-reads", "{T}/r.fa"]

CASES = [
    # ---- the parser: one argv per message
    (HIST + ["-k", "0"], 1, ['<usage>', "Invalid -k '0': k is 1 to 64."]),
    (HIST + ["-k", "65"], 1, ['<usage>', "Invalid -k '65': k is 1 to 64."]),
    (HIST + ["-k", "x"], 1, ['<usage>', "Invalid -k 'x': k is 1 to 64."]),
    (HIST + ["-k"], 1, ['<usage>', "Invalid -k '': k is 1 to 64."]),
    (["-spectrum", "-sequence", "a", "-readmers", "r", "-output", "o", "-copies", "7"], 1, ['<usage>', "Invalid -copies '7': an integer from 1 to 6."]),
    (["-spectrum", "-sequence", "a", "-readmers", "r", "-output", "o", "-copies", "0", "-maxmult", "3"], 1, ['<usage>', "Invalid -copies '0': an integer from 1 to 6.", "Invalid -maxmult '3': an integer from 4 to 65536."]),
    (["-spectrum", "-sequence", "a", "-readmers", "r", "-output", "o", "-maxmult", "65537"], 1, ['<usage>', "Invalid -maxmult '65537': an integer from 4 to 65536."]),
    (["-spectrum", "-sequence", "a", "-readmers", "r", "-output", "o", "-maxmult", "-4"], 1, ['<usage>', "Invalid -maxmult '-4': an integer from 4 to 65536."]),
    (["-spectrum", "-sequence", "a", "-readmers", "r", "-output", "o", "-copies", "2x"], 1, ['<usage>', "Invalid -copies '2x': an integer from 1 to 6."]),
    (["-track", "-sequence", "a", "-readmers", "r", "-output", "o", "-peak", "3", "-window", "0"], 1, ['<usage>', "Invalid -window '0': a window is an integer of at least 1."]),
    (["-track", "-sequence", "a", "-readmers", "r", "-output", "o", "-peak", "3", "-window", "-5"], 1, ['<usage>', "Invalid -window '-5': a window is an integer of at least 1."]),
    (["-track", "-sequence", "a", "-readmers", "r", "-output", "o", "-peak", "3", "-window", "1e3"], 1, ['<usage>', "Invalid -window '1e3': a window is an integer of at least 1."]),
    (["-track", "-sequence", "a", "-readmers", "r", "-output", "o", "-peak", "3", "-window", "99999999999999999999999"], 1, ['<usage>', "Invalid -window '99999999999999999999999': a window is an integer of at least 1."]),
    (HIST + ["-devices", "0-x"], 1, ['<usage>', "Invalid device list '0-x' (-devices 0-7 or 0,2,5)."]),
    (HIST + ["-devices", "3-1"], 1, ['<usage>', "Invalid device list '3-1' (-devices 0-7 or 0,2,5)."]),
    (HIST + ["-devices", ""], 1, ['<usage>', "Invalid device list '' (-devices 0-7 or 0,2,5)."]),
    (HIST + ["-devices", "0,,1"], 1, ['<usage>', "Invalid device list '0,,1' (-devices 0-7 or 0,2,5)."]),
    (HIST + ["-devices", "-1"], 1, ['<usage>', "Invalid device list '-1' (-devices 0-7 or 0,2,5)."]),
    (HIST + ["-devices", "0;1"], 1, ['<usage>', "Invalid device list '0;1' (-devices 0-7 or 0,2,5)."]),
    (HIST + ["-devices", "a"], 1, ['<usage>', "Invalid device list 'a' (-devices 0-7 or 0,2,5)."]),
    (HIST + ["-devices"], 1, ['<usage>', "Invalid device list '' (-devices 0-7 or 0,2,5)."]),
    (HIST + ["-bogus"], 1, ['<usage>', "Unknown option '-bogus'."]),
    (["-bogus", "-sequence", "a", "-output", "o", "-readmers", "r", "-peak", "3"], 1, ['<usage>', "Unknown option '-bogus'.", 'No report type (-filter, -polish, -hist, -dump, -completeness) supplied.']),      # unknown option + no report type
    (["-bogus", "-completeness", "-readmers", "x", "-peak", "3"], 1, ['<usage>', "Unknown option '-bogus'.", 'No sequence meryl database (-seqmers) nor sequence (-sequence) supplied.']),
    # ---- -passes
    (COUNT + ["-passes", "0"], 1, ['<usage>', "Invalid -passes '0': -count takes at least one pass (1 to 4096, or auto)."]),
    (COUNT + ["-passes", "4097"], 1, ['<usage>', "Invalid -passes '4097': a pass takes at least one of the 4096 key bins, so there are 4096 at most (or auto)."]),
    (COUNT + ["-passes", "x"], 1, ['<usage>', "Invalid -passes 'x': the passes of -count are a number from 1 to 4096, or auto."]),
    (COUNT + ["-passes", "-2"], 1, ['<usage>', "Invalid -passes '-2': -count takes at least one pass (1 to 4096, or auto)."]),
    (COUNT + ["-passes", ""], 1, ['<usage>', "Invalid -passes '': the passes of -count are a number from 1 to 4096, or auto."]),
    (COUNT + ["-passes", "3", "-passes", "0", "-k", "99"], 1, ['<usage>', "Invalid -passes '0': -count takes at least one pass (1 to 4096, or auto).", "Invalid -k '99': k is 1 to 64."]),
    (HIST + ["-passes", "0"], 1, ['<usage>', "Invalid -passes '0': -count takes at least one pass (1 to 4096, or auto).", '-passes divides the work of -count: it has no meaning without -count.']),
    (HIST + ["-passes", "4097"], 1, ['<usage>', "Invalid -passes '4097': a pass takes at least one of the 4096 key bins, so there are 4096 at most (or auto).", '-passes divides the work of -count: it has no meaning without -count.']),
    (HIST + ["-passes", "x"], 1, ['<usage>', "Invalid -passes 'x': the passes of -count are a number from 1 to 4096, or auto.", '-passes divides the work of -count: it has no meaning without -count.']),
    (HIST + ["-passes", "auto"], 1, ['<usage>', '-passes divides the work of -count: it has no meaning without -count.']),
    (HIST + ["-passes", "4"], 1, ['<usage>', '-passes divides the work of -count: it has no meaning without -count.']),
    # ---- -count: every flag it refuses, one at a time, then all at once (the order)
    (["-count"], 1, ['<usage>', '-count needs the reads it counts: give -reads <file> (repeatable).', '-count needs -k: no database gives it.', '-count writes a k-mer database: give -output <file>.']),
    (COUNT + ["-convert", "db"], 1, ['<usage>', '-count and -convert are two operations: give one of them.']),
    (COUNT + ["-hist"], 1, ['<usage>', '-count is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).']),
    (["-count", "-k", "21", "-output", "{T}/o.mfxk"], 1, ['<usage>', '-count needs the reads it counts: give -reads <file> (repeatable).']),
    (["-count", "-reads", "{T}/r.fa", "-output", "{T}/o.mfxk"], 1, ['<usage>', '-count needs -k: no database gives it.']),
    (["-count", "-reads", "{T}/r.fa", "-k", "21"], 1, ['<usage>', '-count writes a k-mer database: give -output <file>.']),
    (["-count", "-reads", "{T}/r.fa", "-k", "32", "-output", "{T}/o.mfxk"], 1, ['<usage>', '-count holds k <= 31 (here k = 32): count larger k-mers with `meryl count` and give the database as -readmers.']),
    (COUNT + ["-readmers", "r"], 1, ['<usage>', '-count makes the read database: it does not take -readmers.']),
    (COUNT + ["-seqmers", "s"], 1, ['<usage>', '-count counts reads: it does not take -seqmers.']),
    (COUNT + ["-sequence", "a"], 1, ['<usage>', '-count counts reads: it does not take -sequence.']),
    (COUNT + ["-vcf", "v"], 1, ['<usage>', '-count does not take -vcf (the variant modes do).']),
    (COUNT + ["-peak", "3"], 1, ['<usage>', '-count evaluates nothing: it does not take -peak.']),
    (COUNT + ["-peak", "auto"], 1, ['<usage>', '-count evaluates nothing: it does not take -peak.']),
    (COUNT + ["-sharded"], 1, ['<usage>', '-count does not take -sharded: the table it counts into lives on one device.']),
    (COUNT + ["-index", "i"], 1, ['<usage>', '-count does not take -index: it writes a database, not a table image.']),
    (COUNT + ["-devices", "0,1"], 1, ['<usage>', '-count runs on one device (-device d, or -devices naming one).']),
    (["-count", "-reads", "{T}/none.fa", "-k", "21", "-output", "{T}/o.mfxk"], 1, ['<usage>', "Cannot read the -reads file '{T}/none.fa'."]),
    (["-count", "-reads", "{T}", "-reads", "{T}/r.fa", "-reads", "{T}/none.fa", "-k", "21", "-output", "{T}/o.mfxk"], 1, ['<usage>', "Cannot read the -reads file '{T}'.", "Cannot read the -reads file '{T}/none.fa'."]),
    (["-count", "-convert", "db", "-dump", "-k", "40", "-readmers", "r", "-seqmers", "s", "-sequence", "a", "-vcf", "v", "-peak", "3", "-sharded", "-index", "i",
      "-devices", "0-3", "-passes", "9999", "-window", "5", "-copies", "3"], 1, ['<usage>', "Invalid -passes '9999': a pass takes at least one of the 4096 key bins, so there are 4096 at most (or auto).", '-count and -convert are two operations: give one of them.', '-count is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).', '-count needs the reads it counts: give -reads <file> (repeatable).', '-count writes a k-mer database: give -output <file>.', '-count holds k <= 31 (here k = 40): count larger k-mers with `meryl count` and give the database as -readmers.', '-count makes the read database: it does not take -readmers.', '-count counts reads: it does not take -seqmers.', '-count counts reads: it does not take -sequence.', '-count does not take -vcf (the variant modes do).', '-count evaluates nothing: it does not take -peak.', '-count does not take -sharded: the table it counts into lives on one device.', '-count does not take -index: it writes a database, not a table image.', '-count runs on one device (-device d, or -devices naming one).']),
    (["-count", "-reads", "{T}/none.fa", "-polish", "-bogus", "-skipMissing"], 1, ['<usage>', "Unknown option '-bogus'.", '-count is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).', '-count needs -k: no database gives it.', '-count writes a k-mer database: give -output <file>.', "Cannot read the -reads file '{T}/none.fa'."]),
    # ---- -reads
    (["-convert", "db", "-output", "o", "-reads", "{T}/r.fa", "-k", "21"], 1, ['<usage>', '-convert rewrites a k-mer database; it does not take -reads.', 'No input sequences (-sequence) supplied.', 'No haploid peak (-peak) supplied.', 'No report type (-filter, -polish, -hist, -dump, -completeness) supplied.']),
    (READS + ["-k", "21", "-readmers", "r"], 1, ['<usage>', '-reads and -readmers cannot be combined: the read counts come from one source.']),
    (["-completeness", "-sequence", "a", "-peak", "3", "-reads", "{T}/r.fa", "-k", "21"], 1, ['<usage>', '-completeness needs every read k-mer: it takes a read database (-readmers), not -reads.']),
    (READS + ["-k", "21", "-sharded", "-devices", "0,1"], 1, ['<usage>', '-sharded does not take -reads (give the read database with -readmers).']),
    (READS, 1, ['<usage>', '-reads needs -k (or -seqmers, whose k it then takes).']),
    (["-hist", "-sequence", "a", "-output", "o", "-peak", "3", "-reads", "{T}/none.fa", "-k", "21"], 1, ['<usage>', "Cannot read the -reads file '{T}/none.fa'."]),
    (["-polish", "-sequence", "a", "-output", "o", "-peak", "3", "-vcf", "v", "-reads", "{T}/r.fa", "-k", "21", "-index", "i"], 1, ['<usage>', 'The variant modes count -reads into the path-only index of the call set: one device, no -index.']),
    (["-filter", "-sequence", "a", "-output", "o", "-vcf", "v", "-reads", "{T}/r.fa", "-k", "21", "-devices", "0,0"], 1, ['<usage>', 'The variant modes count -reads into the path-only index of the call set: one device, no -index.']),
    (["-polish", "-sequence", "a", "-output", "o", "-peak", "3", "-vcf", "v", "-reads", "{T}/r.fa", "-k", "33"], 1, ['<usage>', 'The variant modes count -reads into the path-only index, which holds k <= 31 (here k = 33).']),
    (READS + ["-k", "21", "-seqmers", "{T}/asm.txt"], 1, ['<usage>', '-k 21 disagrees with -seqmers, which holds 5-mers.']),
    (["-completeness", "-readmers", "r", "-reads", "{T}/none.fa", "-reads", "{T}/r.fa", "-sharded", "-convert", "db", "-peak", "3"], 1, ['<usage>', '-convert rewrites a k-mer database; it does not take -reads.', '-reads and -readmers cannot be combined: the read counts come from one source.', '-completeness needs every read k-mer: it takes a read database (-readmers), not -reads.', '-sharded does not take -reads (give the read database with -readmers).', '-reads needs -k (or -seqmers, whose k it then takes).', "Cannot read the -reads file '{T}/none.fa'.", 'No sequence meryl database (-seqmers) nor sequence (-sequence) supplied.']),
    (["-strict", "-sequence", "a", "-output", "o", "-peak", "3", "-vcf", "v", "-reads", "{T}/none.fa", "-k", "40", "-index", "i", "-readmers", "r"], 1, ['<usage>', '-reads and -readmers cannot be combined: the read counts come from one source.', "Cannot read the -reads file '{T}/none.fa'.", 'The variant modes count -reads into the path-only index of the call set: one device, no -index.', 'The variant modes count -reads into the path-only index, which holds k <= 31 (here k = 40).']),
    (HIST + ["-k", "21"], 1, ['<usage>', '-k is taken from -readmers; give -k only with -reads.']),
    # ---- -track
    (HIST + ["-window", "500"], 1, ['<usage>', '-window sets the window of -track; it has no meaning without -track.']),
    (["-track", "-sequence", "a", "-readmers", "r", "-output", "o", "-peak", "3", "-sharded"], 1, ['<usage>', "-track does not take -sharded: a window's records need every k-mer's counts on one device."]),
    (["-track", "-sequence", "a", "-readmers", "r", "-output", "o", "-peak", "3", "-devices", "0,1"], 1, ['<usage>', '-track runs on one device (-device d, or -devices naming one).']),
    (["-track", "-sequence", "a", "-readmers", "r", "-output", "o", "-peak", "3", "-skipMissing"], 1, ['<usage>', '-skipMissing belongs to -dump; -track always writes its windows.']),
    (["-track", "-sequence", "a", "-readmers", "r", "-output", "o", "-peak", "3", "-vcf", "v"], 1, ['<usage>', '-track does not take -vcf (the variant modes do).']),
    (["-track", "-sharded", "-devices", "0-1", "-skipMissing", "-vcf", "v", "-window", "x"], 1, ['<usage>', "Invalid -window 'x': a window is an integer of at least 1.", "-track does not take -sharded: a window's records need every k-mer's counts on one device.", '-track runs on one device (-device d, or -devices naming one).', '-skipMissing belongs to -dump; -track always writes its windows.', '-track does not take -vcf (the variant modes do).', 'No input sequences (-sequence) supplied.', 'No output (-output) supplied.', 'No haploid peak (-peak) supplied.', 'No read meryl database (-readmers) supplied.']),
    # ---- -spectrum
    (HIST + ["-copies", "3"], 1, ['<usage>', '-copies and -maxmult shape the image of -spectrum; they have no meaning without -spectrum.']),
    (HIST + ["-maxmult", "100"], 1, ['<usage>', '-copies and -maxmult shape the image of -spectrum; they have no meaning without -spectrum.']),
    (["-spectrum", "-sequence", "a", "-readmers", "r", "-output", "o", "-vcf", "v"], 1, ['<usage>', '-spectrum does not take -vcf (the variant modes do).']),
    (["-spectrum", "-sequence", "a", "-readmers", "r", "-output", "o", "-sharded"], 1, ['<usage>', '-spectrum does not take -sharded: this version counts the spectrum of one table on one device.']),
    (["-spectrum", "-sequence", "a", "-readmers", "r", "-output", "o", "-devices", "0,1"], 1, ['<usage>', '-spectrum runs on one device (-device d, or -devices naming one).']),
    (["-spectrum", "-sequence", "a", "-readmers", "r", "-output", "o", "-skipMissing"], 1, ['<usage>', '-skipMissing belongs to -dump; -spectrum counts every entry of the table.']),
    (["-spectrum", "-readmers", "r", "-output", "o"], 1, ['<usage>', 'No sequence meryl database (-seqmers) nor sequence (-sequence) supplied.']),
    (["-spectrum", "-seqmers", "s", "-reads", "{T}/r.fa", "-k", "21", "-output", "o"], 1, ["ERROR: opening -seqmers: k-mer database 's' does not exist"]),
    (["-spectrum", "-seqmers", "{T}/asm.txt", "-reads", "{T}/r.fa", "-output", "o"], 1, ['<usage>', '-spectrum counts -reads into the k-mers of -sequence: give -sequence.']),
    (["-spectrum", "-readmers", "r"], 1, ['<usage>', 'No sequence meryl database (-seqmers) nor sequence (-sequence) supplied.', 'No output (-output) supplied.']),
    (["-spectrum", "-vcf", "v", "-sharded", "-devices", "0,1", "-skipMissing", "-reads", "{T}/r.fa", "-k", "21"], 1, ['<usage>', '-sharded does not take -reads (give the read database with -readmers).', '-spectrum does not take -vcf (the variant modes do).', '-spectrum does not take -sharded: this version counts the spectrum of one table on one device.', '-spectrum runs on one device (-device d, or -devices naming one).', '-skipMissing belongs to -dump; -spectrum counts every entry of the table.', 'No sequence meryl database (-seqmers) nor sequence (-sequence) supplied.', '-spectrum counts -reads into the k-mers of -sequence: give -sequence.', 'No output (-output) supplied.']),
    # ---- -peak auto
    (HIST + ["-peak", "auto"], 1, ['<usage>', '-peak was given twice (a number and auto).']),
    (["-hist", "-sequence", "a", "-output", "o", "-readmers", "r", "-peak", "auto", "-peak", "3"], 1, ['<usage>', '-peak was given twice (a number and auto).']),
    (["-polish", "-sequence", "a", "-output", "o", "-readmers", "r", "-vcf", "v", "-peak", "auto"], 1, ['<usage>', '-peak auto reads the peak off the table of -hist, -dump, -track or -spectrum; the variant modes and -completeness take -peak <number>.']),
    (["-completeness", "-seqmers", "s", "-readmers", "r", "-peak", "auto"], 1, ['<usage>', '-peak auto reads the peak off the table of -hist, -dump, -track or -spectrum; the variant modes and -completeness take -peak <number>.']),
    (["-hist", "-sequence", "a", "-output", "o", "-readmers", "r", "-peak", "auto", "-sharded"], 1, ['<usage>', '-peak auto does not take -sharded: no peak is defined on a sharded table.']),
    (["-hist", "-sequence", "a", "-output", "o", "-readmers", "r", "-peak", "auto", "-devices", "0,1"], 1, ['<usage>', '-peak auto runs on one device (-device d, or -devices naming one).']),
    (["-filter", "-peak", "2", "-peak", "auto", "-sharded", "-devices", "0,1"], 1, ['<usage>', '-peak was given twice (a number and auto).', '-peak auto reads the peak off the table of -hist, -dump, -track or -spectrum; the variant modes and -completeness take -peak <number>.', '-peak auto does not take -sharded: no peak is defined on a sharded table.', '-peak auto runs on one device (-device d, or -devices naming one).', 'No input sequences (-sequence) supplied.', 'No output (-output) supplied.', 'No variant call input (-vcf) supplied; mandatory for -filter or -polish.', 'No read meryl database (-readmers) supplied.']),
    (["-peak", "auto"], 1, ['<usage>', 'No input sequences (-sequence) supplied.', 'No output (-output) supplied.', 'No report type (-filter, -polish, -hist, -dump, -completeness) supplied.', 'No read meryl database (-readmers) supplied.']),
    # ---- what every report needs
    ([], 1, ['<usage>', 'No input sequences (-sequence) supplied.', 'No output (-output) supplied.', 'No haploid peak (-peak) supplied.', 'No report type (-filter, -polish, -hist, -dump, -completeness) supplied.', 'No read meryl database (-readmers) supplied.']),
    (["-hist"], 1, ['<usage>', 'No input sequences (-sequence) supplied.', 'No output (-output) supplied.', 'No haploid peak (-peak) supplied.', 'No read meryl database (-readmers) supplied.']),
    (["-dump", "-readmers", "r", "-peak", "3", "-output", "o"], 1, ['<usage>', 'No input sequences (-sequence) supplied.']),
    (["-dump", "-readmers", "r", "-peak", "3", "-sequence", "a"], 1, ['<usage>', 'No output (-output) supplied.']),
    (["-spectrum", "-sequence", "a", "-readmers", "r"], 1, ['<usage>', 'No output (-output) supplied.']),
    (["-polish", "-sequence", "a", "-output", "o", "-readmers", "r", "-peak", "3"], 1, ['<usage>', 'No variant call input (-vcf) supplied; mandatory for -filter or -polish.']),
    (["-filter", "-sequence", "a", "-output", "o", "-readmers", "r"], 1, ['<usage>', 'No variant call input (-vcf) supplied; mandatory for -filter or -polish.']),
    (["-better", "-sequence", "a", "-output", "o", "-readmers", "r", "-vcf", "v"], 1, ['<usage>', 'No haploid peak (-peak) supplied.']),
    (["-loose"], 1, ['*EXPERIMENTAL* Running in -loose mode', '<usage>', 'No input sequences (-sequence) supplied.', 'No output (-output) supplied.', 'No variant call input (-vcf) supplied; mandatory for -filter or -polish.', 'No haploid peak (-peak) supplied.', 'No read meryl database (-readmers) supplied.']),
    (["-completeness", "-readmers", "r", "-peak", "3"], 1, ['<usage>', 'No sequence meryl database (-seqmers) nor sequence (-sequence) supplied.']),
    (["-completeness", "-seqmers", "s", "-peak", "3"], 1, ['<usage>', 'No read meryl database (-readmers) supplied.']),
    (["-sequence", "a", "-output", "o", "-readmers", "r", "-peak", "3"], 1, ['<usage>', 'No report type (-filter, -polish, -hist, -dump, -completeness) supplied.']),
    (["-hist", "-sequence", "a", "-output", "o", "-peak", "3"], 1, ['<usage>', 'No read meryl database (-readmers) supplied.']),
    # ---- -convert
    (["-convert", "db"], 1, ['No output (-output) supplied.']),
    (["-convert", "db", "-placed"], 1, ['No output (-output) supplied.']),
    (["-convert", "db", "-bogus"], 1, ['<usage>', "Unknown option '-bogus'.", 'No input sequences (-sequence) supplied.', 'No output (-output) supplied.', 'No haploid peak (-peak) supplied.', 'No report type (-filter, -polish, -hist, -dump, -completeness) supplied.', 'No read meryl database (-readmers) supplied.']),
    (["-convert", "db", "-output", "o", "-window", "3"], 1, ['<usage>', '-window sets the window of -track; it has no meaning without -track.', 'No input sequences (-sequence) supplied.', 'No haploid peak (-peak) supplied.', 'No report type (-filter, -polish, -hist, -dump, -completeness) supplied.', 'No read meryl database (-readmers) supplied.']),
]


def run_case(argv, tmp):
    (tmp / "r.fa").write_text(">r0\nACGTACGTACGTACGTACGTACGTACGT\n")
    (tmp / "asm.txt").write_text("AAAAC\t1\nAAAAG\t2\n")
    r = subprocess.run([EXE] + [a.replace("{T}", str(tmp)) for a in argv], capture_output=True, text=True)
    err = r.stderr.replace(str(tmp), "{T}")
    a, b = err.find("usage: "), err.find(USAGE_END)
    if a < 0:
        return r.returncode, err.splitlines(), None
    assert b > a, err
    usage = err[a:b + len(USAGE_END)].replace(EXE, "merfin")
    return r.returncode, err[:a].splitlines() + ["<usage>"] + err[b + len(USAGE_END):].splitlines(), zlib.crc32(usage.encode())


@pytest.mark.parametrize("case", range(len(CASES)))
def test_cli_refusal(tmp_path, case):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    argv, code, lines = CASES[case]
    got_code, got_lines, crc = run_case(argv, tmp_path)
    assert (got_code, got_lines) == (code, lines), argv
    assert crc in (None, USAGE_CRC)
    assert not any("HIP device" in l for l in got_lines)          # refused before a device is asked for


if __name__ == "__main__":
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        for argv, _, _ in CASES:
            code, lines, crc = run_case(argv, pathlib.Path(d))
            print("    (%r, %r, %r),  # usage crc %r" % (argv, code, lines, crc))
