"""-hist over one sequence held in every form the library keeps a resident sequence in, on every -hist route of the narrow kernels.

A sequence the library made its own copy of (Sequences.from_device, the one-byte-per-base upload of a small assembly) gets its
packed planes once, where the copy is made; its launches then copy their tiles instead of encoding them from the bytes.
MFX_SEQ_PACK=0 keeps the bytes.  Here the same contigs are evaluated
  * from_device (planes), from_device under MFX_SEQ_PACK=0 (bytes), the host upload (planes), and a packed streamed run,
  * on k = 21 compact (four and five minimizer windows), k = 31 quotient form, k = 22 and k = 19 (generic compact instance), and the
    full table,
and every source must give the oracle's integers and, among the sources, the SAME koverCpy bit for bit (one kernel, the same
(tile, wave) words, summed in a fixed order).

The contigs sit around every boundary of the tile and of a wave's share of it: lengths k - 1 .. k + 1, 64, 127 .. 129, 255 .. 257,
511 .. 513, 1023 .. 1025, 4095 .. 4097, 4096 + k - 2, 4096 + k - 1, 8192 + 5 (so consecutive tiles change contig, and the last
tile of a contig is short or holds no k-mer at all); N at 63, 64, 127, 128, 1023, 1024, 4095, 4096 and at those -+ (k - 1);
lower-case stretches, one across a tile seam; a repeated unit (assembly counts above readK: koverCpy terms), once across a seam;
for even k, k-mers that are their own reverse complement at and across the seams.

koverCpy against the oracle: the device's value is within (n_under + (4 ntiles + 64) S) 2^-53 of the exact sum S of the terms
(tests/test_gpu_kstar_grid.py derives it); n_under <= kasm.  The oracle's value is a sequential fp64 sum of at most kasm terms, every
addition rounding by at most 2^-53 of a partial sum <= S: within kasm S 2^-53 of S.  The bar is the sum of the two."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import synth
from tests.test_gpu_parity import assert_hist_equal, build_index, oracle_hist
from tests.test_gpu_seqonly import seq_index

pytestmark = pytest.mark.gpu

PEAK = 17.3
TILE = 4096
MARKS = (63, 64, 127, 128, 1023, 1024, 4095, 4096)
# route -> (k, index kind, environment while the index is made)
ROUTES = {"k21": (21, "seq", {}), "k21_w5": (21, "seq", {"MFX_MZ_W": "5"}), "k31": (31, "seq", {}), "k22": (22, "seq", {}), "k19": (19, "seq", {}),
          "k21_full": (21, "full", {})}
_RC = bytes.maketrans(b"ACGT", b"TGCA")
_worlds = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _lens(k):
    return [k - 1, k, k + 1, 64, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1,
            8192 + 5, 8192 + 5, 8192 + 5, 8192 + 5]


def _contigs(k, seed):
    r = synth.rng(seed)
    lens = _lens(k)
    c = [synth.random_contig(r, n) for n in lens]
    long0 = lens.index(8192 + 5)                               # the plain long contig; the three behind it carry the N marks
    unit = synth.random_contig(r, 300)
    for ci, at in ((lens.index(4097), 3600), (lens.index(4096 + k - 1), 3800), (long0, 6000), (long0 + 1, 2000), (long0 + 3, 5000)):
        c[ci][at:at + 300] = unit                              # (3800 + 300 > 4096: one copy lies across the seam)
    if k % 2 == 0:
        for at in (64 - k // 2, 128, 1024 - 3, TILE - k + 1, TILE + 1):       # (TILE - k + 1: its last base is the next tile's first)
            h = synth.random_contig(r, k // 2).tobytes()
            c[long0][at:at + k] = np.frombuffer(h + h.translate(_RC)[::-1], dtype=np.uint8)
    for j, shift in enumerate((0, -(k - 1), k - 1)):
        for p in MARKS:
            c[long0 + 1 + j][p + shift] = ord("N")
    c[long0][500:620] |= 0x20
    c[long0 + 3][TILE - 16:TILE + 14] |= 0x20                  # lower case across the seam (N -> n: still no base)
    return synth.as_bytes(c)


def _tables(k, contigs, seed):
    r = synth.rng(seed)
    ak, av = po.count_kmers(k, contigs)
    rv = r.poisson(PEAK, size=len(ak)).astype(np.uint64)       # whatever the assembly count: a repeated k-mer has asmK > readK
    rv[r.random(len(ak)) < 0.03] = 0                           # missing from the reads
    big = r.random(len(ak)) < 0.02
    rv[big] = r.choice([2046, 2047, 2048, 70000], size=int(big.sum()))      # around and beyond the compact layout's 11-bit fields
    keep = rv > 0
    return (ak[keep], rv[keep].astype(np.uint32)), (ak, av)


def _world(k):
    """one world and its oracle result per k, shared by every test here; unchanged"""
    if k not in _worlds:
        contigs = _contigs(k, 7100 + k)
        read, asm = _tables(k, contigs, 7200 + k)
        _, g, ka, km = oracle_hist(k, PEAK, contigs, read, asm)
        assert g.kmissing > 100 and g.koverCpy > 100.0
        _worlds[k] = (contigs, read, asm, g, ka, km)
    return _worlds[k]


def _ntiles(contigs):
    return sum((len(c) + TILE - 1) // TILE for c in contigs)


def kover_bar(g, ntiles):
    S = g.koverCpy * (1.0 + 2.0 ** -40)
    return (g.kasm + (4 * ntiles + 64) * S + g.kasm * S) * 2.0 ** -53


def _from_device(m, contigs):
    """(sequence object, the caller's tensors): the tensors are zeroed before return -- the library evaluates ITS copy"""
    import torch
    dev = [torch.frombuffer(bytearray(c), dtype=torch.uint8).cuda() for c in contigs]
    s = m.Sequences.from_device([t.data_ptr() for t in dev], [len(c) for c in contigs])
    for t in dev:
        t.zero_()
    torch.cuda.synchronize()
    return s


def _sources(m, contigs, monkeypatch):
    packed = _from_device(m, contigs)
    upload = m.Sequences(contigs)                              # far below the packed transport's size: bytes over the bus, planes on the device
    monkeypatch.setenv("MFX_SEQ_PACK", "0")
    plain = _from_device(m, contigs)
    plain_upload = m.Sequences(contigs)
    monkeypatch.delenv("MFX_SEQ_PACK")
    assert packed.packed and upload.packed and not plain.packed and not plain_upload.packed
    assert packed.ntiles == plain.ntiles == _ntiles(contigs)
    return {"from_device": packed, "from_device MFX_SEQ_PACK=0": plain, "upload": upload, "upload MFX_SEQ_PACK=0": plain_upload}


def _index(m, route, monkeypatch, seqs):
    k, kind, env = ROUTES[route]
    contigs, read, asm, g, ka, km = _world(k)
    for a, b in env.items():
        monkeypatch.setenv(a, b)
    if kind == "seq":
        ix, _ = seq_index(m, k, contigs, read, asm, seqs=seqs)        # claimed from the packed sequence: the claim kernel copies its tiles too
        assert ix.info()["compact"] and ix.info()["seq_only"]
    else:
        ix = build_index(m, k, read, asm)
    for a in env:
        monkeypatch.delenv(a)
    return ix


def _assert_same(a, b, what):
    assert (a.kasm, a.kmissing) == (b.kasm, b.kmissing), what
    np.testing.assert_array_equal(a.undr(), b.undr(), err_msg=what)
    np.testing.assert_array_equal(a.over(), b.over(), err_msg=what)
    np.testing.assert_array_equal(a.contig_kasm(), b.contig_kasm(), err_msg=what)
    np.testing.assert_array_equal(a.contig_kmissing(), b.contig_kmissing(), err_msg=what)
    assert np.float64(a.koverCpy).tobytes() == np.float64(b.koverCpy).tobytes(), (what, a.koverCpy, b.koverCpy)


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_source_of_the_sequence_gives_the_oracles_result(route, monkeypatch):
    m = _mfx()
    k, kind, _ = ROUTES[route]
    contigs, read, asm, g, ka, km = _world(k)
    src = _sources(m, contigs, monkeypatch)
    ix = _index(m, route, monkeypatch, src["from_device"])
    ev = m.Evaluator(ix, m.KParams(PEAK))
    res = {name: ev.hist(s) for name, s in src.items()}              # (a sequence-only index accepts them all: one content digest, whatever the form)
    res["streamed, packed"] = ev.hist_streamed(m.Sequences.create([len(c) for c in contigs]), contigs)
    res["from_device again"] = ev.hist(src["from_device"])
    bar = kover_bar(g, _ntiles(contigs))
    for name, r in res.items():
        err = abs(r.koverCpy - g.koverCpy)
        print("%s / %s: kasm %d kmissing %d koverCpy %.17g, |gpu - oracle| %.3e (bar %.3e)" % (route, name, r.kasm, r.kmissing, r.koverCpy, err, bar))
        assert_hist_equal(r, g, ka, km, k)
        assert err <= bar, (route, name, err, bar)
        _assert_same(r, res["from_device"], "%s / %s" % (route, name))
    for s in src.values():
        assert s.packed == (s in (src["from_device"], src["upload"]))        # evaluating changes nobody's form


def test_a_streamed_run_of_bytes_into_a_packed_sequence_drops_its_planes(monkeypatch):
    """MFX_STREAM_ASCII=1 writes d_bases: the planes made at the copy are not the sequence any more"""
    m = _mfx()
    k = 21
    contigs, read, asm, g, ka, km = _world(k)
    other = synth.as_bytes(synth.mutate(synth.rng(5), [np.frombuffer(c, dtype=np.uint8) for c in contigs], sub_rate=0.02))
    assert other != contigs
    _, g2, ka2, km2 = oracle_hist(k, PEAK, other, read, asm)
    assert g2.kmissing > g.kmissing
    ev = m.Evaluator(build_index(m, k, read, asm), m.KParams(PEAK))
    s = _from_device(m, contigs)
    assert s.packed
    assert_hist_equal(ev.hist(s), g, ka, km, k)
    monkeypatch.setenv("MFX_STREAM_ASCII", "1")
    assert_hist_equal(ev.hist_streamed(s, other), g2, ka2, km2, k)
    monkeypatch.delenv("MFX_STREAM_ASCII")
    assert not s.packed
    assert_hist_equal(ev.hist(s), g2, ka2, km2, k)                   # the resident launch reads what the streamed run wrote
    s.pack()
    assert s.packed
    assert_hist_equal(ev.hist(s), g2, ka2, km2, k)
    assert_hist_equal(ev.hist_streamed(s, contigs), g, ka, km, k)    # a packed streamed run: the planes are the sequence again
    assert s.packed
    assert_hist_equal(ev.hist(s), g, ka, km, k)


def _image(m, ev, launch, ncontigs):
    import torch
    counts = torch.zeros(m.hist_words(ev.nbins, ncontigs), dtype=torch.int64, device="cuda")
    kover = torch.zeros(1, dtype=torch.float64, device="cuda")
    launch(counts, kover, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert len(ev.take_overflow()) == 0                              # (no K* bin beyond the dense image in this world)
    return counts.cpu().numpy().view(np.uint64), float(kover.item())


@pytest.mark.parametrize("route", ["k21", "k31"])
def test_launch_ranges_and_cyclic_shares(route, monkeypatch):
    """a launch whose next tile is not tile + 1 (the cyclic shares of 3 ranks, blocks of 1 and 2 tiles) and launches that end inside the
    sequence ([0, 1), [1, 3), [T - 1, T)): planes == bytes in every word of the image and in koverCpy's bits; the parts sum to the whole"""
    m = _mfx()
    k, kind, _ = ROUTES[route]
    contigs, read, asm, g, ka, km = _world(k)
    src = _sources(m, contigs, monkeypatch)
    packed, plain = src["from_device"], src["from_device MFX_SEQ_PACK=0"]
    ev = m.Evaluator(_index(m, route, monkeypatch, packed), m.KParams(PEAK))
    T, nc = packed.ntiles, len(contigs)
    assert T > 8
    whole, kwhole = _image(m, ev, lambda c, kv, st: ev.hist_launch(packed, 0, T, c, kv, stream=st), nc)
    assert_hist_equal(ev.result_from_counts(whole, kwhole, nc), g, ka, km, k)
    tot, ktot = np.zeros_like(whole), 0.0
    for lo, hi in ((0, 1), (1, 3), (3, T - 1), (T - 1, T)):
        a, kva = _image(m, ev, lambda c, kv, st: ev.hist_launch(packed, lo, hi, c, kv, stream=st), nc)
        b, kvb = _image(m, ev, lambda c, kv, st: ev.hist_launch(plain, lo, hi, c, kv, stream=st), nc)
        np.testing.assert_array_equal(a, b, err_msg="tiles [%d, %d)" % (lo, hi))
        assert np.float64(kva).tobytes() == np.float64(kvb).tobytes(), (lo, hi, kva, kvb)
        tot += a
        ktot += kva
    np.testing.assert_array_equal(tot, whole)
    assert abs(ktot - kwhole) <= kover_bar(g, T)
    for bt in (1, 2):
        tot, ktot = np.zeros_like(whole), 0.0
        for rank in range(3):
            a, kva = _image(m, ev, lambda c, kv, st: ev.hist_launch_cyclic(packed, rank, 3, c, kv, block_tiles=bt, stream=st), nc)
            b, kvb = _image(m, ev, lambda c, kv, st: ev.hist_launch_cyclic(plain, rank, 3, c, kv, block_tiles=bt, stream=st), nc)
            np.testing.assert_array_equal(a, b, err_msg="rank %d of 3, blocks of %d" % (rank, bt))
            assert np.float64(kva).tobytes() == np.float64(kvb).tobytes(), (rank, bt, kva, kvb)
            assert a[2 * ev.nbins + 0] > 0                           # every share holds k-mers
            tot += a
            ktot += kva
        np.testing.assert_array_equal(tot, whole, err_msg="blocks of %d" % bt)
        assert abs(ktot - kwhole) <= kover_bar(g, T)


def test_small_worklist_segments_from_the_planes(monkeypatch):
    """the worklist forced small (segments of 3 entries: most rare endings fall back to the lane's own scan): the listed entries' terms land
    in the (tile, wave) words of the tiles the planes were copied from -- the result is the default's, bit for bit"""
    m = _mfx()
    k = 21
    contigs, read, asm, g, ka, km = _world(k)
    src = _sources(m, contigs, monkeypatch)
    ev = m.Evaluator(_index(m, "k21", monkeypatch, src["from_device"]), m.KParams(PEAK))
    base = ev.hist(src["from_device"])
    assert_hist_equal(base, g, ka, km, k)
    assert ev.debug_worklist_read()[2].sum() > 0                     # the default list is in use in this world (saturated counts)
    ev.debug_worklist(2, 3)
    for name in ("from_device", "from_device MFX_SEQ_PACK=0"):
        _assert_same(ev.hist(src[name]), base, name)
        segs, segcap, counts, _ = ev.debug_worklist_read()
        assert segcap == 3 and counts.max() == 3
    ev.debug_worklist(1)
