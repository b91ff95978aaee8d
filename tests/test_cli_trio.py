"""`merfin -trio -mat m -pat p [-child c] -output stem [-cutmat n|auto] [-cutpat n|auto] [-cutchild n|auto] [-maxmult M]` and
`merfin -histogram db -output file [-maxmult M]`: every flag check fails with return code 1 and its own message before any device is
touched (runs on a host without a GPU); the usage names the two only for a command line that names one of their flags, behind the usage
text that was there, which stays byte for byte.  The files are checked on the GPU (tests/test_gpu_cli_trio.py)."""
import os

import numpy as np
import pytest

from tests.test_cli import EXE, run

ENTRY = "  Hap-mer databases of a trio, and k-mer histograms (operations of their own: no -sequence, no -readmers, no -peak):\n"
HIST = ["-hist", "-sequence", "asm.fa", "-readmers", "reads.meryl", "-peak", "26", "-output", "out"]
SEPARATE = "%s, -bin, -phase, -count, -convert and -merge are separate operations: give one of them.\n"


def _db(path, k, kmers):
    import merfin_amd as m
    kmers = np.array(sorted(kmers), dtype=np.uint64)
    m.db_write_flat(str(path), k, kmers, np.ones(len(kmers), dtype=np.uint32))
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("trio")
    return {"M": _db(d / "m.mfxk", 21, [5, 9, 77]), "P": _db(d / "p.mfxk", 21, [6, 9]), "C": _db(d / "c.mfxk", 21, [5, 6, 8]), "dir": d}


def _trio(f, *extra):
    return ["-trio", "-mat", f["M"], "-pat", f["P"], "-child", f["C"], "-output", str(f["dir"] / "out")] + list(extra)


def _histo(f, *extra):
    return ["-histogram", f["M"], "-output", str(f["dir"] / "out.hist")] + list(extra)


def _cases(f):
    M, P, C = f["M"], f["P"], f["C"]
    out = str(f["dir"] / "out")
    gone = str(f["dir"] / "gone.mfxk")
    cases = [
        (["-trio", "-pat", P, "-output", out], ["-trio needs the maternal database: give -mat <file>.\n"]),
        (["-trio", "-mat", M, "-output", out], ["-trio needs the paternal database: give -pat <file>.\n"]),
        (["-trio", "-mat", M, "-pat", P], ["-trio writes <output>.hapA.mfxk and <output>.hapB.mfxk: give -output <stem>.\n"]),
        (["-trio"], ["-trio needs the maternal database: give -mat <file>.\n", "-trio needs the paternal database: give -pat <file>.\n",
                     "-trio writes <output>.hapA.mfxk and <output>.hapB.mfxk: give -output <stem>.\n"]),
        (["-trio", "-mat", M, "-pat", P, "-output", out, "-cutchild", "3"], ["-cutchild sets the cutoff of the child's database: it has no meaning without -child.\n"]),
        (["-trio", "-mat", M, "-pat", P, "-output", out, "-cutchild", "auto"], ["-cutchild sets the cutoff of the child's database: it has no meaning without -child.\n"]),
        (_trio(f, "-mat", gone), ["Cannot read the -mat database '%s'.\n" % gone]),
        (_trio(f, "-child", gone), ["Cannot read the -child database '%s'.\n" % gone]),
        (HIST + ["-mat", M], ["-mat names the maternal database of -trio; it has no meaning without -trio.\n"]),
        (HIST + ["-pat", P], ["-pat names the paternal database of -trio; it has no meaning without -trio.\n"]),
        (HIST + ["-child", C], ["-child names the child's database of -trio; it has no meaning without -trio.\n"]),
        (HIST + ["-cutmat", "3"], ["-cutmat, -cutpat and -cutchild set the cutoffs of -trio; they have no meaning without -trio.\n"]),
        # -trio and -histogram with another mode
        (_trio(f, "-hist"), ["-trio is an operation of its own: it does not take a report type (-hist, -dump, -completeness, -spectrum, ...).\n"]),
        (_trio(f, "-spectrum"), ["-trio is an operation of its own: it does not take a report type (-hist, -dump, -completeness, -spectrum, ...).\n"]),
        (_trio(f, "-merge", M), [SEPARATE % "-trio"]),
        (_trio(f, "-count"), [SEPARATE % "-trio"]),
        (_trio(f, "-convert", M), [SEPARATE % "-trio"]),
        (_trio(f, "-phase"), [SEPARATE % "-trio"]),
        (_trio(f, "-bin"), [SEPARATE % "-trio"]),
        (_trio(f, "-histogram", M), ["-trio and -histogram are two operations: give one of them.\n"]),
        (_trio(f, "-join"), ["-join is a way to run -completeness and -spectrum: -trio does not take it.\n"]),
        (_trio(f, "-readmers", "r.meryl"), ["-trio takes its databases by flags of its own: it does not take -readmers.\n"]),
        (_trio(f, "-seqmers", "s.meryl"), ["-trio takes its databases by flags of its own: it does not take -seqmers.\n"]),
        (_trio(f, "-sequence", "asm.fa"), ["-trio evaluates nothing: it does not take -sequence.\n"]),
        (_trio(f, "-reads", "r.fq"), ["-trio reads databases: it does not take -reads (count them first: -count).\n"]),
        (_trio(f, "-peak", "26"), ["-trio evaluates no K*: it does not take -peak.\n"]),
        (_trio(f, "-vcf", "x.vcf"), ["-trio does not take -vcf (the variant modes do).\n"]),
        (_trio(f, "-sharded", "-devices", "0,1"), ["-trio does not take -sharded: the windows it reads live on one device.\n",
                                                   "-trio runs on one device (-device d, or -devices naming one).\n"]),
        (_trio(f, "-index", "i"), ["-trio does not take -index: it builds no table.\n"]),
        (_trio(f, "-copies", "3"), ["-copies shapes the image of -spectrum: -trio does not take it.\n"]),
        (_trio(f, "-maxmult", "3"), ["Invalid -maxmult '3': an integer from 4 to 65536.\n"]),
        (_histo(f, "-hist"), ["-histogram is an operation of its own: it does not take a report type (-hist, -dump, -completeness, -spectrum, ...).\n"]),
        (_histo(f, "-merge", M), [SEPARATE % "-histogram"]),
        (_histo(f, "-bin"), [SEPARATE % "-histogram"]),
        (_histo(f, "-mat", M), ["-mat, -pat, -child and the cutoffs belong to -trio: -histogram takes one database, -histogram <file>.\n"]),
        (_histo(f, "-cutmat", "2"), ["-mat, -pat, -child and the cutoffs belong to -trio: -histogram takes one database, -histogram <file>.\n"]),
        (["-histogram", M], ["-histogram writes a k-mer histogram: give -output <file>.\n"]),
        (["-histogram", gone, "-output", out], ["Cannot read the -histogram database '%s'.\n" % gone]),
        (_histo(f, "-peak", "auto"), ["-histogram evaluates no K*: it does not take -peak.\n"]),
        (_histo(f, "-devices", "0,1"), ["-histogram runs on one device (-device d, or -devices naming one).\n"]),
    ]
    for flag in ("-cutmat", "-cutpat", "-cutchild"):
        for bad in ("0", "-1", "1.5", "x", "", "Auto", "4294967296"):
            cases.append((_trio(f, flag, bad), ["Invalid %s '%s': a cutoff of -trio is a count from 1 to 4294967295, or auto.\n" % (flag, bad)]))
    return cases


N_CASES = 40 + 21


@pytest.mark.parametrize("case", range(N_CASES))
def test_trio_refusal(case, files):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    cases = _cases(files)
    assert len(cases) == N_CASES
    argv, lines = cases[case]
    r = run(argv)
    assert r.returncode == 1, r.stderr
    assert r.stderr.startswith("usage: ")
    head, sep, tail = r.stderr.partition(ENTRY)
    assert sep, r.stderr                                       # the command line names a flag of -trio / -histogram: their entries follow the usage
    _, _, mine = tail.partition("\n\n")
    assert mine.splitlines(keepends=True) == lines, r.stderr  # these lines and no other
    assert "ERROR: HIP device" not in r.stderr                # no device was opened
    for name in ("out.hapA.mfxk", "out.hapB.mfxk", "out.trio.stats", "out.hist", "out.hapA.mfxk.blocks"):
        assert not os.path.exists(str(files["dir"] / name))


def test_clean_lines_trip_no_check(files):
    """each check has its own message: a clean line gets past all of them and stops at the device that is not there (on a machine that
    has one it runs)"""
    for argv, done in ((_trio(f := files, "-cutmat", "2", "-cutpat", "auto", "-cutchild", "1", "-maxmult", "50", "-devices", "0", "-output", str(files["dir"] / "clean1")),
                        "-- Cutoffs: mat 2, pat "),
                       (["-trio", "-mat", f["M"], "-pat", f["P"], "-output", str(f["dir"] / "clean2"), "-cutmat", "1", "-cutpat", "4294967295"], "pat 4294967295."),
                       (_histo(f, "-maxmult", "50", "-device", "0", "-output", str(f["dir"] / "clean3.hist")), " k-mers; ")):
        r = run(argv)
        assert not r.stderr.startswith("usage: ") and ENTRY not in r.stderr, r.stderr
        assert (r.returncode == 1 and "ERROR: HIP device 0 not available" in r.stderr) or (r.returncode in (0, 1) and done in r.stderr) or "-trio:" in r.stderr, r.stderr


def test_usage_names_trio_only_when_asked_for():
    plain = run([])
    assert plain.returncode == 1
    for flag in ("-trio", "-histogram", "-cutmat", "-mat ", "-child"):
        assert flag not in plain.stderr
    asked = run(["-trio"])
    assert asked.returncode == 1
    head, sep, tail = asked.stderr.partition(ENTRY)
    assert sep and "    -trio " in tail and "    -mat db / -pat db " in tail and "    -cutmat n|auto " in tail and "    -histogram db " in tail and "    -maxmult M " in tail
    assert "<output>.hapA.mfxk" in tail and "<output>.hapB.mfxk" in tail and "<output>.trio.stats" in tail and "<output>.mat_only.hist" in tail
    assert "not validated against Merqury" in tail and "GenomeScope" in tail
    assert head == plain.stderr[:plain.stderr.index("No input sequences")]      # the usage text that was there, byte for byte, comes first
    assert run(["-histogram"]).stderr.partition(ENTRY)[1]
    # the other operations' entries stay where they were, and theirs do not name -trio
    for argv in (["-merge", "a", "-bogus"], ["-regions"], ["-phase"], ["-bin"], HIST + ["-join"]):
        assert "-trio" not in run(argv).stderr and "-histogram" not in run(argv).stderr
    # -maxmult without -spectrum, -trio or -histogram is still refused as before
    r = run(HIST + ["-maxmult", "50"])
    assert r.stderr.endswith("\n\n-copies and -maxmult shape the image of -spectrum; they have no meaning without -spectrum.\n") and ENTRY not in r.stderr
