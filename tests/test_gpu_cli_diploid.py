"""`merfin -diploid` end to end on the GPU, on one world of three blocks: the four files it writes against tests/diploid_ref.py;
<output>.spectra-cn.hist byte for byte the file of `merfin -merge hap1 hap2` followed by `merfin -spectrum -join`; and with -peak the
completeness lines on stderr those of three `merfin -completeness -join` runs, on hap1, on hap2 and on the merged database."""
import math

import pytest

from tests import diploid_ref as dr
from tests.test_cli import run
from tests.test_diploid_cpu import BIG, three

pytestmark = pytest.mark.gpu

K = 21
_world = {}


def _files(tmp_path_factory):
    """the three sorted flat files and the merged assembly's, written once"""
    if not _world:
        import merfin_amd as m
        if m.device_count() < 1:
            pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
        d = tmp_path_factory.mktemp("diploid")
        world = three(K, (BIG, 2 * 4096 + 10, 4097), 42)
        names = [str(d / n) for n in ("read.mfxk", "h1.mfxk", "h2.mfxk")]
        for p, (keys, vals) in zip(names, world):
            m.db_write_flat(p, K, keys, vals)
        r = run(["-merge", names[1], "-merge", names[2], "-output", str(d / "M.mfxk")])
        assert r.returncode == 0, r.stderr
        _world.update(d=d, world=world, names=names + [str(d / "M.mfxk")])
    return _world["d"], _world["world"], _world["names"]


def _completeness_lines(stderr):
    return [l for l in stderr.splitlines() if l.startswith(("thread ", "TOTAL ", "COMPLETENESS:"))]


def _rows(text):
    return [l.split("\t") for l in text.splitlines() if not l.startswith("#")]


def test_the_four_files(tmp_path_factory, tmp_path, monkeypatch):
    d, world, (rp, p1, p2, mp) = _files(tmp_path_factory)
    for i, extra in enumerate(([], ["-copies", "2", "-maxmult", "20", "-min", "2", "-max", "30"])):
        monkeypatch.setenv("MFX_MERGE_RANGE", "3000") if i else monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
        stem, chain = str(tmp_path / ("d%d" % i)), str(tmp_path / ("j%d" % i))
        r = run(["-diploid", "-readmers", rp, "-hap1", p1, "-hap2", p2, "-output", stem] + extra)
        assert r.returncode == 0, r.stderr
        assert r.stderr.rstrip().endswith("Bye!")
        want = dr.diploid(*world, K, copies=2, max_mult=20, lo=2, hi=30) if extra else dr.diploid(*world, K)
        st = want["stats"]
        assert "-- Joined: %d read k-mers, %d and %d assembly k-mers, %d in both assemblies, " % (st["n_read"], st["n_hap1"], st["n_hap2"], st["n_shared"]) in r.stderr
        # spectra-cn: the bytes of the chain
        j = run(["-spectrum", "-join", "-readmers", rp, "-seqmers", mp, "-output", chain] + extra)
        assert j.returncode == 0, j.stderr
        assert open(stem + ".spectra-cn.hist", "rb").read() == open(chain + ".spectra-cn.hist", "rb").read()
        # spectra-asm: the class image, non-zero cells only
        lines = open(stem + ".spectra-asm.hist").read().splitlines()
        assert lines[0] == "Assembly\tkmer_multiplicity\tCount"
        cells = [(row, col) for row in range(4) for col in range(want["asm_img"].shape[1]) if want["asm_img"][row, col]]
        labels = ("read-only", "hap1-only", "hap2-only", "shared")
        assert lines[1:] == ["%s\t%d\t%d" % (labels[row], col, want["asm_img"][row, col]) for row, col in cells] and len(cells) > 8
        # qv: the total counts, then the distinct ones
        rows = _rows(open(stem + ".qv").read())
        assert [x[0] for x in rows] == ["hap1", "hap2", "both"] * 2
        for n, x in enumerate(rows):
            c = st[x[0]]
            only, total = (c["only_total"], c["total"]) if n < 3 else (c["only_distinct"], c["distinct"])
            assert (int(x[1]), int(x[2])) == (only, total) and only > 0
            err = 1.0 - (1.0 - only / total) ** (1.0 / K)
            assert abs(float(x[3]) - -10.0 * math.log10(err)) < 1e-3 and abs(float(x[4]) - err) <= 1e-5 * err
        assert "unvalidated against Merqury" in open(stem + ".qv").read() and "unvalidated against Merqury" in open(stem + ".completeness.stats").read()
        # completeness.stats
        rows = _rows(open(stem + ".completeness.stats").read())
        assert [(x[0], x[1], int(x[2]), int(x[3])) for x in rows] == [(name, "all", st[name]["found"], st["solid"]) for name in dr.NAMES]
        assert all(abs(float(x[4]) - 100.0 * int(x[2]) / int(x[3])) < 1e-3 for x in rows)


def test_peak_prints_the_three_completeness_reports(tmp_path_factory, tmp_path, monkeypatch):
    d, world, (rp, p1, p2, mp) = _files(tmp_path_factory)
    monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
    (tmp_path / "prob.txt").write_text("1,0.5\n1,1.0\n2,0.25\n0,0.0\n")
    for extra in ([], ["-prob", str(tmp_path / "prob.txt")]):
        want = []
        for ap in (p1, p2, mp):
            j = run(["-completeness", "-join", "-readmers", rp, "-seqmers", ap, "-peak", "17.3"] + extra)
            assert j.returncode == 0, j.stderr
            want += _completeness_lines(j.stderr)
        assert len(want) == 3 * (64 + 3)
        r = run(["-diploid", "-readmers", rp, "-hap1", p1, "-hap2", p2, "-output", str(tmp_path / "p"), "-peak", "17.3"] + extra)
        assert r.returncode == 0, r.stderr
        assert _completeness_lines(r.stderr) == want
        heads = [l for l in r.stderr.splitlines() if l.startswith("-- Compute completeness: ")]
        assert heads == ["-- Compute completeness: %s." % n for n in dr.NAMES]
