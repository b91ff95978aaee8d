"""`merfin -spectrum [-copies C] [-maxmult M]` and `-peak auto`: every flag check fails with return code 1 and its message
before any device is touched (runs on a host without a GPU); the images, the files and the peak are checked on the GPU
(tests/test_gpu_spectrum.py, tests/test_gpu_cli_spectrum.py)."""
import os

from tests.test_cli import EXE, run

IN = ["-sequence", "asm.fa", "-readmers", "reads.meryl", "-output", "out"]


def _spec(*extra):
    return ["-spectrum"] + IN + list(extra)


def _refused(args, msg):
    r = run(args)
    assert r.returncode == 1 and msg in r.stderr, (args, r.stderr[-600:])
    assert "ERROR: HIP device" not in r.stderr                 # no device was opened
    return r


def test_spectrum_flag_validation():
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    _refused(_spec("-vcf", "calls.vcf"), "-spectrum does not take -vcf (the variant modes do).\n")
    _refused(_spec("-sharded", "-devices", "0,1"), "-spectrum does not take -sharded: this version counts the spectrum of one table on one device.\n")
    r = _refused(_spec("-devices", "0,1"), "-spectrum runs on one device (-device d, or -devices naming one).\n")
    assert "-spectrum does not take -sharded" not in r.stderr
    _refused(_spec("-window", "500"), "-window sets the window of -track; it has no meaning without -track.\n")
    _refused(_spec("-skipMissing"), "-skipMissing belongs to -dump; -spectrum counts every entry of the table.\n")
    for flag, val in (("-copies", "3"), ("-maxmult", "500")):
        _refused(["-hist", "-peak", "26"] + IN + [flag, val],
                 "-copies and -maxmult shape the image of -spectrum; they have no meaning without -spectrum.\n")
    for bad in ("0", "7", "-1", "x", "", "2.5", "+3", " 3", "99999999999999999999999"):
        _refused(_spec("-copies", bad), "Invalid -copies '%s': an integer from 1 to 6.\n" % bad)
    for bad in ("0", "3", "65537", "-4", "x", "", "1e3", "99999999999999999999999"):
        _refused(_spec("-maxmult", bad), "Invalid -maxmult '%s': an integer from 4 to 65536.\n" % bad)
    _refused(["-spectrum", "-sequence", "asm.fa", "-readmers", "reads.meryl"], "No output (-output) supplied.\n")
    _refused(["-spectrum", "-readmers", "reads.meryl", "-output", "out"], "No sequence meryl database (-seqmers) nor sequence (-sequence) supplied.\n")
    _refused(["-spectrum", "-sequence", "asm.fa", "-output", "out"], "No read meryl database (-readmers) supplied.\n")


def test_peak_auto_flag_validation():
    for mode in ("-filter", "-polish", "-better", "-strict", "-loose", "-completeness"):
        _refused([mode, "-vcf", "calls.vcf", "-peak", "auto"] + IN,
                 "-peak auto reads the peak off the table of -hist, -dump, -track or -spectrum; the variant modes and -completeness take -peak <number>.\n")
    for mode in ("-hist", "-dump", "-track", "-spectrum"):
        _refused([mode, "-peak", "auto", "-sharded", "-devices", "0,1"] + IN, "-peak auto does not take -sharded: no peak is defined on a sharded table.\n")
        _refused([mode, "-peak", "auto", "-devices", "0-2"] + IN, "-peak auto runs on one device (-device d, or -devices naming one).\n")
    _refused(["-hist", "-peak", "auto", "-peak", "26"] + IN, "-peak was given twice (a number and auto).\n")
    # a -peak that is neither a number nor auto stays what it was: no peak
    _refused(["-hist", "-peak", "Auto"] + IN, "No haploid peak (-peak) supplied.\n")


def test_clean_lines_pass_validation():
    """-spectrum needs no -peak, and -peak auto stands for one: such a line trips no check -- it stops later, at the device or at the database that is not there"""
    lines = [_spec(), _spec("-copies", "1", "-maxmult", "4"), _spec("-copies", "6", "-maxmult", "65536", "-devices", "0"), _spec("-peak", "auto"),
             _spec("-peak", "26", "-prob", "table.txt"), _spec("-min", "2", "-max", "2500", "-memory", "10", "-index", "img"),
             ["-spectrum", "-seqmers", "asm.meryl", "-readmers", "reads.meryl", "-output", "out"]]
    lines += [[mode, "-peak", "auto"] + IN for mode in ("-hist", "-dump", "-track")]
    for args in lines:
        r = run(args)
        assert r.returncode == 1 and "usage:" not in r.stderr, (args, r.stderr[-600:])
        for msg in ("No haploid peak", "Invalid -", "-spectrum does not", "-spectrum runs", "-peak auto", "-copies and", "Unknown option"):
            assert msg not in r.stderr, (args, r.stderr)


def test_usage_names_the_new_flags():
    r = run([])
    assert r.returncode == 1
    for s in ("    -spectrum ", "    -copies C ", "    -maxmult M ", "    -peak auto ", "<output>.spectra-cn.hist"):
        assert s in r.stderr, s
    # the lines that were there stay
    assert "    -track          K* summarised per window of every contig on the GPU" in r.stderr
    assert "No report type (-filter, -polish, -hist, -dump, -completeness) supplied." in r.stderr
