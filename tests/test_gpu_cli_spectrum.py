"""`merfin -spectrum` and `-peak auto` end to end on the GPU: the report byte for byte against tests/spectrum_ref.py, and a run
with -peak auto against the same run with the peak written out."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import spectrum_ref as sr
from tests import synth
from tests import synth_reads
from tests.test_cli import _write_fasta, run

pytestmark = pytest.mark.gpu

W21 = dict(k=21, peak=17.3, seed=42, sizes=(120000, 9000, 4096, 4097, 500, 20, 0, 8191))
W31 = dict(k=31, peak=17.3, seed=44, sizes=(60000, 20000, 4097, 30, 0))
_worlds = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _world(tmp_path_factory, name, spec):
    """the FASTA file and the read database of a world, written once; (directory, contigs, read, asm)"""
    if name not in _worlds:
        m = _mfx()
        d = tmp_path_factory.mktemp(name)
        contigs, read, asm = synth.world(**spec)
        _write_fasta(str(d / "asm.fasta"), contigs)
        m.db_write_flat(str(d / "read.mfxk"), spec["k"], *read)
        _worlds[name] = (d, contigs, read, asm)
    return _worlds[name]


def test_spectrum_from_a_read_database(tmp_path, tmp_path_factory):
    d, contigs, read, asm = _world(tmp_path_factory, "w21", W21)
    out = str(tmp_path / "o")
    r = run(["-spectrum", "-sequence", str(d / "asm.fasta"), "-readmers", str(d / "read.mfxk"), "-output", out])
    assert r.returncode == 0, r.stderr
    img = sr.image(read, asm, 4, 10000)
    assert open(out + ".spectra-cn.hist").read() == sr.text(img, True)
    assert "Entries counted: %d\n" % int(img.sum()) in r.stderr
    assert "Assembly-only k-mers: %d\n" % int(img[1:, 0].sum()) in r.stderr and "Read-only k-mers: %d\n" % int(img[0].sum()) in r.stderr
    v, p, h, n = sr.peak(img[1])
    assert (v, p, h) == (1, 17, 17)
    assert "Haploid peak (auto): %d  (main peak %d, valley %d, single-copy k-mers at the peak %d)\n" % (h, p, v, n) in r.stderr
    assert r.stderr.rstrip().endswith("Bye!")
    # -copies / -maxmult / -min / -max
    r = run(["-spectrum", "-sequence", str(d / "asm.fasta"), "-readmers", str(d / "read.mfxk"), "-output", out + "2", "-copies", "2", "-maxmult", "20",
             "-min", "2", "-max", "30"])
    assert r.returncode == 0, r.stderr
    assert open(out + "2.spectra-cn.hist").read() == sr.text(sr.image(read, asm, 2, 20, 2, 30), True)


def test_spectrum_from_reads(tmp_path):
    k = 21
    asm, reads = synth_reads.reads_world(k, 721)
    fa, rq = str(tmp_path / "asm.fasta"), str(tmp_path / "reads.fasta")
    _write_fasta(fa, asm)
    _write_fasta(rq, reads)
    out = str(tmp_path / "o")
    r = run(["-spectrum", "-sequence", fa, "-reads", rq, "-k", str(k), "-output", out])
    assert r.returncode == 0, r.stderr
    img = sr.image(po.count_kmers(k, reads), po.count_kmers(k, asm), 4, 10000, seq_only=True)
    assert not img[0].any()
    text = open(out + ".spectra-cn.hist").read()
    assert text == sr.text(img, False) and "read-only" not in text
    assert "the read-only row is left out" in r.stderr and "Read-only k-mers:" not in r.stderr


def _strip(stderr):
    return [l for l in stderr.splitlines() if not l.startswith("Haploid peak (auto)")]


@pytest.mark.parametrize("mode,world", [("-hist", "w21"), ("-dump", "w31"), ("-track", "w31")])
def test_peak_auto_equals_the_peak_written_out(mode, world, tmp_path, tmp_path_factory):
    d, contigs, read, asm = _world(tmp_path_factory, world, W21 if world == "w21" else W31)
    args = [mode, "-sequence", str(d / "asm.fasta"), "-readmers", str(d / "read.mfxk"), "-output", "out"] + (["-window", "1000"] if mode == "-track" else [])
    res = {}
    for name, peak in (("auto", "auto"), ("given", "17")):
        cwd = tmp_path / name
        cwd.mkdir()
        res[name] = run(args + ["-peak", peak], cwd=str(cwd))
        assert res[name].returncode == 0, res[name].stderr
    assert sum(l.startswith("Haploid peak (auto): 17  (main peak 17, valley 1, ") for l in res["auto"].stderr.splitlines()) == 1
    assert "Haploid peak" not in res["given"].stderr
    assert _strip(res["auto"].stderr) == res["given"].stderr.splitlines()          # the summary, the per-contig lines
    files = sorted(os.listdir(str(tmp_path / "given")))
    assert files == sorted(os.listdir(str(tmp_path / "auto"))) and len(files) == (3 if mode == "-track" else 1)
    for f in files:
        a, b = (tmp_path / "auto" / f).read_bytes(), (tmp_path / "given" / f).read_bytes()
        assert a == b and len(a) > 0, f                              # (a -hist file of a small world is a few lines)


def test_no_peak_to_find(tmp_path):
    """a Poisson(2.5) world: the single-copy row falls from 2 on -- -peak auto asks for -peak, -spectrum reports and says so"""
    k = 21
    contigs, read, asm = synth.world(k=k, peak=2.5, seed=46, sizes=(1999,) * 10, err_kmers=500)
    assert sr.peak(sr.image(read, asm, 4, 10000, seq_only=True)[1]) is None and sr.peak(sr.image(read, asm, 4, 10000)[1]) is None
    m = _mfx()
    fa, db = str(tmp_path / "asm.fasta"), str(tmp_path / "read.mfxk")
    _write_fasta(fa, contigs)
    m.db_write_flat(db, k, *read)
    r = run(["-hist", "-sequence", fa, "-readmers", db, "-peak", "auto", "-output", str(tmp_path / "o.hist")])
    assert r.returncode == 1 and "ERROR: -peak auto found no haploid peak" in r.stderr and "Give -peak <number>." in r.stderr
    assert not os.path.exists(str(tmp_path / "o.hist"))
    r = run(["-spectrum", "-sequence", fa, "-readmers", db, "-output", str(tmp_path / "o")])
    assert r.returncode == 0, r.stderr
    assert "No haploid peak found in the single-copy row" in r.stderr and "Haploid peak (auto)" not in r.stderr
    assert open(str(tmp_path / "o.spectra-cn.hist")).read() == sr.text(sr.image(read, asm, 4, 10000), True)
