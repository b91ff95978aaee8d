"""`merfin -completeness -join` and `merfin -spectrum -join` end to end on the GPU, on one small world: the completeness lines on stderr and
the bytes of <output>.spectra-cn.hist are those of the same command without -join (the table route), and the spectrum's report those of
tests/spectrum_ref.py."""
import numpy as np
import pytest

from tests import spectrum_ref as sr
from tests import synth
from tests.test_cli import run

pytestmark = pytest.mark.gpu

_world = {}


def _files(tmp_path_factory):
    """a read database and the assembly's, both sorted flat files, written once"""
    if not _world:
        import merfin_amd as m
        if m.device_count() < 1:
            pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
        d = tmp_path_factory.mktemp("join")
        contigs, read, asm = synth.world(k=21, peak=17.3, seed=42, sizes=(60000, 9000, 4097, 500, 20))
        m.db_write_flat(str(d / "read.mfxk"), 21, *read)
        m.db_write_flat(str(d / "asm.mfxk"), 21, *asm)
        _world.update(d=d, read=read, asm=asm)
    return _world["d"], _world["read"], _world["asm"]


def _completeness_lines(stderr):
    return [l for l in stderr.splitlines() if l.startswith(("thread ", "TOTAL ", "COMPLETENESS:"))]


def test_completeness_join_prints_the_table_routes_lines(tmp_path_factory, tmp_path, monkeypatch):
    d, read, asm = _files(tmp_path_factory)
    (tmp_path / "prob.txt").write_text("1,0.5\n1,1.0\n2,0.25\n0,0.0\n")
    base = ["-completeness", "-readmers", str(d / "read.mfxk"), "-seqmers", str(d / "asm.mfxk"), "-peak", "17.3"]
    for extra in ([], ["-prob", str(tmp_path / "prob.txt")]):
        monkeypatch.delenv("MFX_MERGE_RANGE", raising=False)
        table = run(base + extra)
        assert table.returncode == 0, table.stderr
        want = _completeness_lines(table.stderr)
        assert len(want) == 64 + 3
        for rng in (None, "3000"):
            if rng:
                monkeypatch.setenv("MFX_MERGE_RANGE", rng)
            r = run(base + extra + ["-join"])
            assert r.returncode == 0, r.stderr
            assert _completeness_lines(r.stderr) == want
            both = len(np.intersect1d(read[0], asm[0]))
            assert "-- Joined: %d read k-mers, %d assembly k-mers, %d in both, " % (len(read[0]), len(asm[0]), both) in r.stderr
            assert r.stderr.rstrip().endswith("Bye!")


def test_spectrum_join_writes_the_table_routes_bytes(tmp_path_factory, tmp_path):
    d, read, asm = _files(tmp_path_factory)
    base = ["-spectrum", "-readmers", str(d / "read.mfxk"), "-seqmers", str(d / "asm.mfxk")]
    for i, extra in enumerate(([], ["-copies", "2", "-maxmult", "20", "-min", "2", "-max", "30"])):
        t, j = str(tmp_path / ("t%d" % i)), str(tmp_path / ("j%d" % i))
        table = run(base + extra + ["-output", t])
        assert table.returncode == 0, table.stderr
        r = run(base + extra + ["-output", j, "-join"])
        assert r.returncode == 0, r.stderr
        got = open(j + ".spectra-cn.hist", "rb").read()
        assert got == open(t + ".spectra-cn.hist", "rb").read()
        img = sr.image(read, asm, 2, 20, 2, 30) if extra else sr.image(read, asm, 4, 10000)
        assert got.decode() == sr.text(img, True)
        for line in ("Entries counted: ", "Assembly-only k-mers: ", "Read-only k-mers: ", "Haploid peak (auto): ", "No haploid peak found"):
            mine = [l for l in r.stderr.splitlines() if l.startswith(line)]
            assert mine == [l for l in table.stderr.splitlines() if l.startswith(line)], line
            assert mine or line.endswith(("(auto): ", "found"))
