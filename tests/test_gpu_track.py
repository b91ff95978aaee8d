"""Evaluator.track / mfx_track_run: K* per fixed window of every contig, reduced on the device.  The expected records are the
per-position values of the oracle's -dump (oracle.pyoracle.process_dump; the plain-Python restatement oracle/plain.py for
32 <= k <= 64, which the C oracle's 64-bit k-mers cannot hold) reduced per window in Python -- integers for the counts, Python
ints for the sum of K* in units of 2^-52 (tests/track_ref.py).  EVERY field of EVERY record is compared with `==`, min and max
included: there is no tolerance anywhere."""
import os

import numpy as np
import pytest

from oracle import plain
from oracle import pyoracle as po
from tests import synth
from tests import track_ref as tr
from tests.test_gpu_parity import build_index
from tests.test_gpu_seqonly import seq_index
from tests.test_gpu_wide import small_world, build as build_wide

pytestmark = pytest.mark.gpu

SIZES = (120000, 9000, 4096, 4097, 500, 20, 10, 0, 8191)       # > 100 000, shorter than k, empty, one position past a tile
WINDOWS = (1, 7, 63, 64, 65, 1000, 4096, 4097, 100000, 10**6)      # the last: larger than the longest contig


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _prob(golden_dir, use_prob):
    return po.load_kmetric(os.path.join(golden_dir, "example_lookup_table.txt")) if use_prob else (None, None)


def _per_position(k, peak, probK, probP, contigs, read, asm, lo=0, hi=2**64 - 1):
    p = po.Params(k, peak, probK, probP)
    R, A = po.Lookup(k, read[0], read[1], lo, hi), po.Lookup(k, *asm)
    return [tr.per_position_c(po, p, R, A, c) for c in contigs]


def _check(m, ev, seqs, pp, windows=WINDOWS, want_nonfinite=False):
    """every window length: records == the reduced oracle values; totals == -hist's; two runs byte-identical"""
    h = ev.hist(seqs)
    seen_nonfinite = 0
    for W in windows:
        want = tr.reduce_windows(pp, W)
        w, kasm, kmissing = ev.track(seqs, W)
        assert w.dtype == m.TRACK_DTYPE and w.dtype.itemsize == 72
        got = tr.device_records(w)
        assert len(got) == len(want) == sum((len(x[0]) + W - 1) // W for x in pp), W
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (W, i, a, b)
        assert (kasm, kmissing) == (h.kasm, h.kmissing), W
        assert (int(w["n_kmers"].sum(dtype=np.uint64)), int(w["n_missing"].sum(dtype=np.uint64))) == (h.kasm, h.kmissing), W
        assert (w["n_scored"] + w["n_missing"] + w["n_nonfinite"] == w["n_kmers"]).all()
        none = w["n_scored"] == 0
        assert np.isposinf(w["min_kstar"][none]).all() and np.isneginf(w["max_kstar"][none]).all()
        w2, _, _ = ev.track(seqs, W)
        assert w.tobytes() == w2.tobytes(), W
        seen_nonfinite += int(w["n_nonfinite"].sum())
    assert h.kasm > 0
    assert (seen_nonfinite > 0) == want_nonfinite
    return h


@pytest.mark.parametrize("use_prob", [False, True])
@pytest.mark.parametrize("index", ["full", "seq"])
@pytest.mark.parametrize("k", [15, 21, 22, 31])
def test_track_matches_the_reduced_dump(k, index, use_prob, golden_dir):
    m = _mfx()
    peak = 26.0 if use_prob else 17.3
    probK, probP = _prob(golden_dir, use_prob)
    contigs, read, asm = synth.world(k=k, peak=peak, seed=7000 + k, sizes=SIZES)
    assert any(0 < len(c) < k for c in contigs) and any(len(c) == 0 for c in contigs)
    assert any(b"N" * 50 in c for c in contigs) and any(c != c.upper() for c in contigs)
    pp = _per_position(k, peak, probK, probP, contigs, read, asm)
    if index == "full":
        ix, seqs = build_index(m, k, read, asm), m.Sequences(contigs)
    else:
        ix, seqs = seq_index(m, k, contigs, read)
        assert ix.info()["compact"]
    ev = m.Evaluator(ix, m.KParams(peak, probK, probP))
    h = _check(m, ev, seqs, pp)
    assert h.kmissing > 0
    # the records do not depend on the form the sequence is held in: the packed planes give the same bytes
    before = {W: ev.track(seqs, W)[0].tobytes() for W in (7, 1000, 4097)}
    seqs.pack()
    for W, b in before.items():
        assert ev.track(seqs, W)[0].tobytes() == b, W


@pytest.mark.parametrize("k,use_prob", [(33, False), (33, True), (64, False), (64, True)])
def test_track_wide_kmers(k, use_prob, golden_dir):
    m = _mfx()
    peak = 9.0
    probK, probP = _prob(golden_dir, use_prob)
    pk, ppb = (probK.tolist(), probP.tolist()) if use_prob else ([], [])
    contigs, R, A = small_world(k, 800 + k)
    pp = [tr.per_position_plain(plain, k, peak, pk, ppb, c, R, A) for c in contigs]
    ix = build_wide(m, k, R, A)
    ev = m.Evaluator(ix, m.KParams(peak, probK, probP))
    _check(m, ev, m.Sequences([c.encode() for c in contigs]), pp)


def test_track_non_canonical_database():
    """a database of forward-strand k-mers: both strands are probed and summed (merfin-globals.C:107-108)"""
    m = _mfx()
    k = 11
    r = synth.rng(3)
    contigs = synth.as_bytes(synth.decorate(r, synth.make_truth(r, (60000, 2500, 4097, 5, 0))))
    fw = {}
    for c in contigs:
        for _, f, _r in po.kiter(k, c):
            fw[f] = fw.get(f, 0) + 1
    ak = np.array(sorted(fw), dtype=np.uint64)
    av = np.array([fw[x] for x in ak.tolist()], dtype=np.uint32)
    rv = (av * 5 + (ak % 3).astype(np.uint32)).astype(np.uint32)
    ix = build_index(m, k, (ak, rv), (ak, av))
    assert not ix.info()["canonical"]
    pp = _per_position(k, 5.0, None, None, contigs, (ak, rv), (ak, av))
    _check(m, m.Evaluator(ix, m.KParams(5.0)), m.Sequences(contigs), pp)


@pytest.mark.parametrize("k", [6, 22])
def test_track_even_k_palindromes(k):
    m = _mfx()
    contigs, read, asm = synth.world(k=k, peak=3.0, sizes=(30000, 700, 4100, 3, 0), err_kmers=0, tandem=None, seed=31 + k)
    pp = _per_position(k, 3.0, None, None, contigs, read, asm)
    _check(m, m.Evaluator(build_index(m, k, read, asm), m.KParams(3.0)), m.Sequences(contigs), pp, windows=(1, 65, 1000, 4097))


@pytest.mark.parametrize("index", ["full", "seq"])
def test_track_foreign_assembly_database_counts_nonfinite(index):
    """-seqmers of another assembly: k-mers of the sequence with asmV == 0, where getKmetric divides by zero -- counted in
    n_nonfinite and left out of every sum"""
    m = _mfx()
    k, peak = 21, 17.3
    contigs, read, asm = synth.world(k=k, peak=peak, seed=909, sizes=SIZES)
    keep = np.random.default_rng(5).random(len(asm[0])) < 0.9
    foreign = (asm[0][keep], asm[1][keep])
    pp = _per_position(k, peak, None, None, contigs, read, foreign)
    if index == "full":
        ix, seqs = build_index(m, k, read, foreign), m.Sequences(contigs)
    else:
        ix, seqs = seq_index(m, k, contigs, read, foreign)
    _check(m, m.Evaluator(ix, m.KParams(peak)), seqs, pp, want_nonfinite=True)


def test_track_counts_beyond_the_slot_fields_and_the_read_filter():
    """the compact layout keeps 11-bit count fields; larger counts live in the side table.  With -min / -max."""
    m = _mfx()
    k, peak = 21, 26.0
    r = np.random.default_rng(88)
    contigs, read, asm = synth.world(k=k, peak=peak, seed=5105, sizes=(50000, 6000, 4097, 30, 0), err_kmers=1500)
    rv = read[1].astype(np.uint64)
    big = r.random(len(rv)) < 0.03
    rv[big] = r.choice([2046, 2047, 2048, 5000, 200000], size=int(big.sum()))
    read = (read[0], rv.astype(np.uint32))
    av = asm[1].copy()
    av[r.random(len(av)) < 0.01] = 3000
    asm = (asm[0], av)
    for lo, hi in ((0, 2**64 - 1), (2, 2500)):
        pp = _per_position(k, peak, None, None, contigs, read, asm, lo, hi)
        ix, seqs = seq_index(m, k, contigs, read, asm, lo, hi)
        assert ix.info()["compact"]
        _check(m, m.Evaluator(ix, m.KParams(peak)), seqs, pp, windows=(1, 64, 1000, 100000))


def test_window_of_one_equals_the_dump_values(golden_dir):
    m = _mfx()
    k, peak = 21, 26.0
    probK, probP = _prob(golden_dir, True)
    contigs, read, asm = synth.world(k=k, peak=peak, seed=4242, sizes=(30000, 4097, 500, 20, 0))
    kp = m.KParams(peak, probK, probP)
    ix, seqs = seq_index(m, k, contigs, read)
    ev = m.Evaluator(ix, kp)
    w, kasm, kmissing = ev.track(seqs, 1)
    assert len(w) == sum(len(c) for c in contigs)
    o = 0
    ka_sum = km_sum = 0
    for c in range(len(contigs)):
        n = len(contigs[c])
        rv, av, ka, km = ev.dump_values(seqs, c, 0, n)
        ka_sum += ka
        km_sum += km
        valid = tr.valid_starts(contigs[c], k)
        x = w[o:o + n]
        o += n
        assert np.array_equal(x["n_kmers"], valid.astype(np.uint32))
        readK = {int(v): m.getK(kp, int(v), 0)[0] for v in np.unique(rv).tolist()}
        rk = np.array([readK[int(v)] for v in rv.tolist()])
        missing = valid & (rk == 0)
        scored = valid & ~missing & (av != 0)
        assert np.array_equal(x["n_missing"], missing.astype(np.uint32)) and np.array_equal(x["n_scored"], scored.astype(np.uint32))
        assert np.array_equal(x["sum_readK"][scored], rk[scored].astype(np.uint64)) and np.array_equal(x["sum_asmK"][scored], av[scored].astype(np.uint64))
        ks = np.array([m.getKmetric(a, float(b)) for a, b in zip(rk[scored].tolist(), av[scored].tolist())])
        assert np.array_equal(x["min_kstar"][scored], ks) and np.array_equal(x["max_kstar"][scored], ks)
        assert not x["sum_readK"][~scored].any() and not x["sum_asmK"][~scored].any()
    assert (kasm, kmissing) == (ka_sum, km_sum)


def test_track_refusals_and_text(tmp_path):
    m = _mfx()
    k, peak = 21, 17.3
    contigs, read, asm = synth.world(k=k, peak=peak, seed=12, sizes=(9000, 4097, 10, 0))
    seqs = m.Sequences(contigs)
    ix = build_index(m, k, read, asm)
    ev = m.Evaluator(ix, m.KParams(peak))
    with pytest.raises(m.MfxError) as e:
        ev.track(seqs, 0)
    assert e.value.code == -1
    L = m.load_library()
    assert L.mfx_track_num_windows(seqs.h, 0) == 0 and L.mfx_track_num_windows(seqs.h, 1000) == 9 + 5 + 1
    # cap too small
    import ctypes as C
    buf = np.zeros(4, dtype=m.TRACK_DTYPE)
    n, ka, km = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert L.mfx_track_run(ev.h, seqs.h, 1000, C.c_void_p(buf.ctypes.data), 4, C.byref(n), C.byref(ka), C.byref(km)) == -1
    # the text: the formatter of the expected records, byte for byte; a .gz name goes through the compressed writer
    import gzip
    names = ["c%d" % i for i in range(len(contigs))]
    for W in (1000, 4096):
        w, _, _ = ev.track(seqs, W)
        pp = _per_position(k, peak, None, None, contigs, read, asm)
        tsv, bg, _ = tr.format_files(tr.reduce_windows(pp, W), names, [len(c) for c in contigs], W)
        m.track_write(w, seqs, names, W, str(tmp_path / "t.tsv"), str(tmp_path / "t.bedgraph.gz"))
        assert (tmp_path / "t.tsv").read_text() == tsv
        assert gzip.open(tmp_path / "t.bedgraph.gz", "rt").read() == bg
    with pytest.raises(m.MfxError):
        m.track_write(w[:3], seqs, names, W, str(tmp_path / "x.tsv"))
    # a shard of an index cannot answer for a window
    sx = m.Index(k, len(read[0]) + len(asm[0]) + 16)
    sx.set_shard(0, 2)
    sx.add_read(*read)
    sx.add_asm(*asm)
    with pytest.raises(m.MfxError) as e:
        m.Evaluator(sx, m.KParams(peak)).track(seqs, 1000)
    assert e.value.code == -1 and "shard" in str(e.value)
