"""The -dump text writer (dump_contig_impl) across its chunk seams.  Values arrive in chunks of 2**24 positions, double
buffered on a helper thread; host threads format disjoint pieces of a chunk and write them at offsets computed from the
pieces before them.  MFX_DUMP_CHUNK brings the seam -- the buffer swap, the counters added chunk by chunk, the file
offsets carried from chunk to chunk -- within reach of small contigs; one test crosses the real seam at the default.
Everything is compared with the oracle's processDump + outputDump (merfin-dump.C:44-67, 87-93) byte for byte, and with its
(kasm, kmissing)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from oracle import plain
from oracle import pyoracle as po
from tests import dump_ranges as dr
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "merfin_amd", "bin", "merfin")
K = 21


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def world_on_device(tmp_path_factory):
    """the text world on the device, its evaluator under the golden table, and the oracle's text per list of contigs: made once"""
    m = _mfx()
    w = dr.text_world(K)
    prob = dr.golden_table()
    rk, rv = w.arrays(w.read)
    ak, av = w.arrays(w.asm)
    ix = m.Index(K, len(rv) + len(av) + 16)
    ix.add_read(rk, rv)
    ix.add_asm(ak, av)
    ev, seqs = m.Evaluator(ix, m.KParams(dr.PEAK, *prob)), m.Sequences(w.contigs)
    texts, scratch = {}, tmp_path_factory.mktemp("oracle")

    def expected(contigs):
        if tuple(contigs) not in texts:
            texts[tuple(contigs)] = dr.dump_text(w, str(scratch / "oracle.dump"), *prob, contigs=contigs)
        return texts[tuple(contigs)]
    yield m, w, ev, seqs, expected, prob
    ev.close()
    seqs.close()
    ix.close()


def _dump_all(ev, seqs, contigs, path, want):
    for i, c in enumerate(contigs):
        assert ev.dump_contig(seqs, c, dr.name_of(c), path, append=i > 0) == want[c], c


def _set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("MFX_DUMP_CHUNK", raising=False)
    else:
        monkeypatch.setenv("MFX_DUMP_CHUNK", chunk)


@pytest.mark.parametrize("chunk", ["7", "255", "4096", "4097", "10000", None, "1", "0", "4097x", str((1 << 24) + 1)],
                         ids=lambda c: "chunk-%s" % (c or "unset"))
def test_chunk_by_contig_length(chunk, world_on_device, tmp_path, monkeypatch):
    """contigs of 0, 1, k - 1, k, 4096, 4097 and 20011 positions one after another into one file, at every chunk size; a chunk
    of one position only on the contigs under 1000 positions (every chunk is a call with three allocations); 0, malformed and
    too large values mean the default"""
    m, w, ev, seqs, expected, _ = world_on_device
    contigs = [c for c in range(len(w.contigs)) if chunk != "1" or len(w.contigs[c]) < 1000]
    want_text, want = expected(contigs)
    _set_chunk(monkeypatch, chunk)
    monkeypatch.setenv("MFX_HOST_THREADS", "4")              # (2859 chunks of 7 positions: threads are started per chunk)
    path = str(tmp_path / "g.dump")
    _dump_all(ev, seqs, contigs, path, want)
    assert open(path, "rb").read() == want_text
    assert len(want_text) > (400000 if chunk != "1" else 20) and sum(want[c][0] for c in contigs) > 0


@pytest.mark.parametrize("writer", ["positional", "serial", "gz"])
@pytest.mark.parametrize("threads", ["1", "3", "64"])
def test_threads_and_writers_at_a_chunk_of_seven(threads, writer, world_on_device, tmp_path, monkeypatch):
    """1, 3 and 64 formatting threads (64: more threads than positions in a chunk) through the positional writer, the one
    writer of MFX_DUMP_SERIAL=1 and a compressor's pipe"""
    m, w, ev, seqs, expected, _ = world_on_device
    contigs = [1, 2, 3, 5]                                       # 1, k - 1, k and 4097 positions: 586 chunks and the seam of the tile
    want_text, want = expected(contigs)
    monkeypatch.setenv("MFX_DUMP_CHUNK", "7")
    monkeypatch.setenv("MFX_HOST_THREADS", threads)
    if writer == "serial":
        monkeypatch.setenv("MFX_DUMP_SERIAL", "1")
    path = str(tmp_path / ("g.dump.gz" if writer == "gz" else "g.dump"))
    _dump_all(ev, seqs, contigs, path, want)
    got = open(path, "rb").read()
    if writer == "gz":
        assert got[:2] == b"\x1f\x8b"
        got = gzip.decompress(got)
    assert got == want_text and len(want_text) > 80000


@pytest.mark.parametrize("writer", ["positional", "serial"])
@pytest.mark.parametrize("chunk", ["4097", None], ids=["chunk-4097", "chunk-unset"])
def test_append_keeps_and_truncate_drops_what_the_file_held(chunk, writer, world_on_device, tmp_path, monkeypatch):
    m, w, ev, seqs, expected, _ = world_on_device
    want_text, want = expected([6])
    _set_chunk(monkeypatch, chunk)
    if writer == "serial":
        monkeypatch.setenv("MFX_DUMP_SERIAL", "1")
    path = str(tmp_path / "g.dump")
    earlier = b"earlier\tcontent\n" * 3000                      # (longer than a piece of the new text: nothing of it may survive a truncation)
    for append in (True, False):
        with open(path, "wb") as f:
            f.write(earlier)
        assert ev.dump_contig(seqs, 6, dr.name_of(6), path, append=append) == want[6]
        assert open(path, "rb").read() == (earlier if append else b"") + want_text
    short = b"x\n"
    with open(path, "wb") as f:
        f.write(short)
    assert ev.dump_contig(seqs, 0, dr.name_of(0), path, append=True) == (0, 0)      # an empty contig: nothing added
    assert open(path, "rb").read() == short


def test_sharded_text_at_a_chunk_of_4097(world_on_device, tmp_path, monkeypatch):
    from tests.test_gpu_sharded import _build_shards
    m, w, _, seqs, expected, prob = world_on_device
    contigs = list(range(len(w.contigs)))
    want_text, want = expected(contigs)
    evs = [m.Evaluator(ix, m.KParams(dr.PEAK, *prob)) for ix in _build_shards(m, K, w.arrays(w.read), w.arrays(w.asm), 3)]
    monkeypatch.setenv("MFX_DUMP_CHUNK", "4097")
    path = str(tmp_path / "s.dump")
    for c in contigs:
        assert m.dump_contig_sharded(evs, [seqs] * 3, c, dr.name_of(c), path, append=c > 0) == want[c]
    assert open(path, "rb").read() == want_text


def test_cli_dump_end_to_end_at_a_chunk_of_4097(tmp_path):
    _mfx()
    w = dr.text_world(K)
    contigs = [c for c in range(len(w.contigs)) if len(w.contigs[c])]
    want_text, _ = dr.dump_text(w, str(tmp_path / "oracle.dump"), *dr.golden_table(), contigs=contigs)
    with open(tmp_path / "asm.fasta", "wb") as f:
        for c in contigs:
            f.write(b">" + dr.name_of(c).encode() + b" of the text world\n")
            for o in range(0, len(w.contigs[c]), 70):
                f.write(w.contigs[c][o:o + 70] + b"\n")
    for name, table in (("read", w.read), ("asm", w.asm)):
        with open(tmp_path / (name + ".kmers.txt"), "w") as f:
            for x in sorted(table):
                f.write("%s\t%d\n" % (plain.dec(x, K), table[x]))
    common = [EXE, "-dump", "-sequence", str(tmp_path / "asm.fasta"), "-readmers", str(tmp_path / "read.kmers.txt"),
              "-seqmers", str(tmp_path / "asm.kmers.txt"), "-peak", str(dr.PEAK), "-prob", dr.GOLDEN_TABLE]
    out = {}
    for tag, chunk in (("default", None), ("chunked", "4097")):
        env = dict(os.environ)
        env.pop("MFX_DUMP_CHUNK", None)
        if chunk:
            env["MFX_DUMP_CHUNK"] = chunk
        r = subprocess.run(common + ["-output", str(tmp_path / tag)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        out[tag] = (tmp_path / tag).read_bytes()
    assert out["chunked"] == out["default"] == want_text and len(want_text) > 400000


def test_the_real_seam_at_the_default_chunk(tmp_path, monkeypatch):
    """one contig of 2**24 + 4096 + 17 random bases; the database holds the k-mers of three windows -- the first 200 bases, 150
    on either side of position 2**24, the last 300 --, read counts 9 times the assembly counts, peak 9: 740 lines of text, on
    both sides of the chunk seam, and the counters of two chunks added up"""
    m = _mfx()
    monkeypatch.delenv("MFX_DUMP_CHUNK", raising=False)
    CH = 1 << 24
    n = CH + 4096 + 17
    peak = 9.0
    contig = synth.random_contig(synth.rng(424242), n).tobytes()
    windows = [contig[:200], contig[CH - 150:CH + 150], contig[-300:]]
    ak, av = po.count_kmers(K, windows)
    read, asm = (ak, (av * 9).astype(np.uint32)), (ak, av)
    p = po.Params(K, peak)
    rk, akk, kmm, kasm, kmis = po.process_dump(p, po.Lookup(K, *read), po.Lookup(K, *asm), contig)
    opath, gpath = str(tmp_path / "o.dump"), str(tmp_path / "g.dump")
    lines = po.output_dump(opath, "chr", rk, akk, kmm)
    want_text = open(opath, "rb").read()
    pos = [int(l.split(b"\t")[1]) for l in want_text.splitlines()]
    assert lines == len(pos) == 740 and any(CH - 150 <= x < CH for x in pos) and any(CH <= x < CH + 150 for x in pos) and pos[-1] == n - K
    assert kasm == n - K + 1 and kasm - kmis == 740
    ix = m.Index(K, 2 * len(ak) + 16)
    ix.add_read(*read)
    ix.add_asm(*asm)
    ev, seqs = m.Evaluator(ix, m.KParams(peak)), m.Sequences([contig])
    assert ev.dump_contig(seqs, 0, "chr", gpath) == (kasm, kmis)
    assert open(gpath, "rb").read() == want_text
