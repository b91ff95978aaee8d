"""`merfin -track [-window W]`: every flag check fails with return code 1 and its exact message before any device is touched
(runs on a host without a GPU); the records and the files are checked on the GPU (tests/test_gpu_track.py,
tests/test_gpu_cli_track.py)."""
import os

from tests.test_cli import EXE, run


def _base(*extra):
    return ["-track", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26", "-output", "out"] + list(extra)


def test_track_flag_validation():
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    # -window without -track
    r = run(["-hist", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26", "-output", "out", "-window", "500"])
    assert r.returncode == 1 and "-window sets the window of -track; it has no meaning without -track.\n" in r.stderr
    # a -window that is not an integer >= 1
    for bad in ("0", "-5", "1.5", "x", "10k", "", "+7", " 7", "99999999999999999999999"):
        r = run(_base("-window", bad))
        assert r.returncode == 1 and ("Invalid -window '%s': a window is an integer of at least 1.\n" % bad) in r.stderr, bad
    r = run(_base("-sharded", "-devices", "0,1"))
    assert r.returncode == 1 and "-track does not take -sharded: a window's records need every k-mer's counts on one device.\n" in r.stderr
    r = run(_base("-devices", "0,1"))
    assert r.returncode == 1 and "-track runs on one device (-device d, or -devices naming one).\n" in r.stderr
    assert "-track does not take -sharded" not in r.stderr
    r = run(_base("-skipMissing"))
    assert r.returncode == 1 and "-skipMissing belongs to -dump; -track always writes its windows.\n" in r.stderr
    r = run(_base("-vcf", "calls.vcf"))
    assert r.returncode == 1 and "-track does not take -vcf (the variant modes do).\n" in r.stderr
    r = run(["-track", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26"])
    assert r.returncode == 1 and "No output (-output) supplied.\n" in r.stderr
    # each check has its own message: a clean -track line trips none of them (it stops at the missing database instead)
    r = run(_base("-window", "10000", "-devices", "0"))
    for msg in ("-window", "-track does not", "-track runs", "-skipMissing belongs", "No output"):
        assert not any(l.startswith(msg) or l.startswith("Invalid " + msg) for l in r.stderr.splitlines()), r.stderr
    # none of them opened a device
    assert "ERROR: HIP device" not in run(_base("-window", "0")).stderr


def test_usage_names_track_and_window():
    r = run([])
    assert r.returncode == 1
    assert "    -track " in r.stderr and "    -window W " in r.stderr
    assert "<output>.track.tsv" in r.stderr and "<output>.kstar.bedgraph" in r.stderr and "<output>.missing.bedgraph" in r.stderr
    # the lines that were there stay
    assert "    -dump           seqName, seqPos, readK, asmK, K* per k-mer to <output>  [-skipMissing]\n" in r.stderr
    assert "No report type (-filter, -polish, -hist, -dump, -completeness) supplied." in r.stderr
