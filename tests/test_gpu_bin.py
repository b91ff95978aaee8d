"""Evaluator.bin_reads / mfx_bin_*: per-read hap-mer counts made on the device.  The expected rows are the sequential walk of
tests/bin_ref.py over every read (Python integers, two Python sets), computed once per world and shared by the tests that use it.
EVERY field of EVERY record is compared with `==`."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import bin_ref as br
from tests.test_gpu_parity import build_index
from tests.test_gpu_phase import kmers_of
from tests.test_gpu_seqonly import seq_index

pytestmark = pytest.mark.gpu

KS = (6, 15, 16, 21, 22, 31)


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def rnd(r, n):
    return r.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()


def canon(x, k):
    """the canonical form of a k-mer given as an integer (2 bits a base, the complement is ^ 2)"""
    y, r = x, 0
    for _ in range(k):
        r = (r << 2) | ((y & 3) ^ 2)
        y >>= 2
    return min(x, r)


def batches_of(k):
    return (2 * k + 2, max(100, 2 * k + 2), 4096 + 7, 0)


class World:
    """reads of every shape the batcher and the kernel treat differently; two overlapping sets of canonical k-mers taken from them, with
    a few k-mers of neither; the expected rows"""

    def __init__(self, k, seed=0):
        r = np.random.default_rng(9000 + k + seed)
        self.k = k
        reads = [rnd(r, n) for n in (0, k - 1, k, k + 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 5)]
        reads += [b"N" * 40, b"N" * (k + 3), b"n" * 7]                         # reads of only N
        x = bytearray(rnd(r, 700))
        for p in (0, 1, k, 100, 101, 100 + k, 300, 699):                        # N inside a read: at its ends, two of them k apart
            x[p] = ord("N")
        x[400:400 + 2 * k] = b"N" * (2 * k)
        reads.append(bytes(x))
        y = rnd(r, 900)
        reads += [y.lower(), bytes(c | 0x20 if i % 3 else c for i, c in enumerate(y)), y]      # lowercase, mixed case: the k-mers of y again
        reads.append(rnd(r, 3 * 4096 + 11))                                     # one read across three tiles and more
        reads += [rnd(r, k) for _ in range(300)]                                # 300 reads of exactly k, back to back: far more pieces than the LDS table holds
        reads += [rnd(r, 0), rnd(r, 2 * k), rnd(r, 5000)]
        self.reads = reads
        cano, fwd = [], []
        for rd in reads:
            v, f, rc = kmers_of(k, rd)
            cano.append(np.minimum(f, rc)[v])
            fwd.append(f[v])
        self.allk = np.unique(np.concatenate(cano))
        self.fwd = np.unique(np.concatenate(fwd))
        u = r.random(len(self.allk))
        present = set(self.allk.tolist())
        foreign = [x for x in (canon(y, k) for y in r.integers(0, 4**k, 64).tolist()) if x not in present]      # (k = 6: the reads hold nearly every 6-mer; few or none are left)
        self.a = np.unique(np.concatenate([self.allk[u < 0.30], np.array(foreign[0::2], dtype=np.uint64)]))
        self.b = np.unique(np.concatenate([self.allk[(u > 0.20) & (u < 0.50)], np.array(foreign[1::2], dtype=np.uint64)]))
        self.want = np.array(br.counts(reads, k, self.a.tolist(), self.b.tolist()), dtype=np.uint32)
        # the world shows what it is for
        assert self.want[:, 1].sum() > 0 and self.want[:, 2].sum() > 0 and self.want[:, 3].sum() > 0
        assert (self.want[:, 0] == [max(0, len(rd) - k + 1) for rd in reads])[:11].all() and self.want[11:14].sum() == 0
        assert (self.want[15] == self.want[16]).all() and (self.want[15] == self.want[17]).all() and self.want[15, 0] == 900 - k + 1


@functools.lru_cache(maxsize=None)
def world(k):
    return World(k)


def tables(a, b):
    """(k-mers, counts) of the two sets; the counts vary: membership is "value > 0", whatever the value"""
    ak, bk = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return (ak, (1 + np.arange(len(ak)) % 5).astype(np.uint32)), (bk, (1 + np.arange(len(bk)) % 7).astype(np.uint32))


@pytest.mark.parametrize("k", KS)
def test_bin_full_canonical_index_every_batch_size(k):
    m = _mfx()
    w = world(k)
    ra, rb = tables(w.a, w.b)
    ix = build_index(m, k, ra, rb)
    assert ix.info()["canonical"]
    ev = m.Evaluator(ix, m.KParams(1.0))
    for batch in batches_of(k):
        got, st = ev.bin_reads(w.reads, batch, with_stats=True)
        assert got.dtype == np.uint32 and got.shape == (len(w.reads), 4)
        assert np.array_equal(got, w.want), (batch, np.flatnonzero((got != w.want).any(axis=1))[:10])
        assert (got[:, 0] >= got[:, 1:].sum(axis=1)).all()
        # the stats equal the column sums
        assert [st["kmers"], st["a"], st["b"], st["shared"]] == w.want.astype(np.uint64).sum(axis=0).tolist(), batch
        assert st["reads"] == len(w.reads) and st["bases"] == sum(len(x) for x in w.reads)
        # a second run gives the same bytes
        assert ev.bin_reads(w.reads, batch).tobytes() == got.tobytes(), batch


@pytest.mark.parametrize("k", KS)
def test_bin_sequence_only_index_claimed_from_the_reads(k):
    m = _mfx()
    w = world(k)
    ra, rb = tables(w.a, w.b)
    ix, _ = seq_index(m, k, w.reads, ra, rb)
    assert ix.info()["seq_only"] and ix.info()["compact"] and ix.info()["canonical"]
    ev = m.Evaluator(ix, m.KParams(1.0))
    for batch in batches_of(k)[1:]:
        assert np.array_equal(ev.bin_reads(w.reads, batch), w.want), batch


@pytest.mark.parametrize("k", [6, 16, 21])
def test_bin_non_canonical_index(k):
    """sets of k-mers as the reads spell them: both strands are looked up, a k-mer is in a set when either strand's is"""
    m = _mfx()
    w = world(k)
    r = np.random.default_rng(77 + k)
    u = r.random(len(w.fwd))
    a, b = w.fwd[u < 0.25], w.fwd[(u > 0.15) & (u < 0.40)]
    want = np.array(br.counts(w.reads, k, a.tolist(), b.tolist(), canonical=False), dtype=np.uint32)
    assert want[:, 1].sum() > 0 and want[:, 2].sum() > 0 and want[:, 3].sum() > 0
    ix = build_index(m, k, *tables(a, b))
    assert not ix.info()["canonical"]
    ev = m.Evaluator(ix, m.KParams(1.0))
    for batch in (max(100, 2 * k + 2), 4096 + 7, 0):
        assert np.array_equal(ev.bin_reads(w.reads, batch), want), batch


def test_bin_empty_and_foreign_sets():
    m = _mfx()
    k = 21
    w = world(k)
    r = np.random.default_rng(5)
    present = set(w.allk.tolist())
    foreign = np.unique(np.array([x for x in (canon(y, k) for y in r.integers(0, 4**k, 400).tolist()) if x not in present], dtype=np.uint64))
    assert len(foreign) > 300
    none = np.zeros(0, dtype=np.uint64)
    for a, b in ((none, w.b), (foreign[:200], foreign[100:])):
        want = np.array(br.counts(w.reads, k, a.tolist(), b.tolist()), dtype=np.uint32)
        ev = m.Evaluator(build_index(m, k, *tables(a, b)), m.KParams(1.0))
        for batch in (100, 0):
            assert np.array_equal(ev.bin_reads(w.reads, batch), want)
        assert want[:, 1].sum() == 0 and (want[:, 2].sum() > 0) == (len(a) == 0) and want[:, 0].sum() == w.want[:, 0].sum()


def test_bin_return_path_take_one_interleaved_with_add():
    m = _mfx()
    k = 21
    w = world(k)
    ev = m.Evaluator(build_index(m, k, *tables(w.a, w.b)), m.KParams(1.0))
    runs = []
    for _ in range(2):
        b = m.Binner(ev, 4096 + 7)
        rows, added = [], 0
        for o in range(0, len(w.reads), 7):
            b.add(w.reads[o:o + 7])
            added += len(w.reads[o:o + 7])
            assert b.ready() <= added - len(rows)
            for _ in range(3):                                       # fewer takes than adds: records pile up, and stay in order
                got = b.take(1)
                assert len(got) <= 1
                rows += got.tolist()
                assert b.ready() <= added - len(rows)
        assert len(rows) < len(w.reads)
        b.flush()
        assert b.ready() == len(w.reads) - len(rows)
        assert len(b.take(0)) == 0
        while b.ready():
            rows += b.take(1).tolist()
        st = b.end()
        assert rows == w.want.tolist()
        assert [st["kmers"], st["a"], st["b"], st["shared"]] == w.want.astype(np.uint64).sum(axis=0).tolist()
        runs.append(np.array(rows, dtype=np.uint32).tobytes())
    assert runs[0] == runs[1]
    # records never taken are lost, and counted
    b = m.Binner(ev, 100)
    b.add(w.reads)
    st = b.end()
    assert [st["kmers"], st["a"], st["b"], st["shared"]] == w.want.astype(np.uint64).sum(axis=0).tolist() and st["reads"] == len(w.reads)


def test_bin_two_million_bases_of_mixed_reads():
    m = _mfx()
    k = 21
    r = np.random.default_rng(4242)
    genome = rnd(r, 400000)
    reads = []
    total = 0
    while total < 2000000:                                           # short and long reads of one genome: the sets' k-mers come back many times
        n = int(r.choice([30, 150, 151, 250, 1000, 12000, 25000, 60000]))
        p = int(r.integers(0, len(genome) - n))
        reads.append(genome[p:p + n])
        total += n
    v, f, rc = kmers_of(k, genome)
    allk = np.unique(np.minimum(f, rc)[v])
    u = r.random(len(allk))
    a, b = allk[u < 0.02], allk[(u > 0.015) & (u < 0.035)]
    want = np.array(br.counts(reads, k, a.tolist(), b.tolist()), dtype=np.uint32)
    ev = m.Evaluator(build_index(m, k, *tables(a, b)), m.KParams(1.0))
    got, st = ev.bin_reads(reads, 1 << 19, with_stats=True)          # four batches: long reads are cut across them
    assert np.array_equal(got, want)
    assert st["bases"] == total and st["kmers"] == int(want[:, 0].astype(np.uint64).sum()) and st["seconds_kernel"] > 0
    assert np.array_equal(ev.bin_reads(reads), want)                 # the default batch holds them all


def test_bin_refusals():
    m = _mfx()
    L = m.load_library()
    k = 21
    w = world(k)
    ra, rb = tables(w.a, w.b)
    ev = m.Evaluator(build_index(m, k, ra, rb), m.KParams(1.0))
    with pytest.raises(m.MfxError) as e:                             # a null argument
        m.Binner(None)
    assert e.value.code == -1 and "null" in str(e.value)
    assert L.mfx_bin_add(None, None, None, 0) == -1 and L.mfx_bin_flush(None) == -1 and L.mfx_bin_end(None, None) == -1
    assert L.mfx_bin_ready(None) == 0 and L.mfx_bin_take(None, None, 0, None) == -1
    with pytest.raises(m.MfxError) as e:                             # a batch below the counters' minimum
        m.Binner(ev, 2 * k + 1)
    assert e.value.code == -1 and "too small" in str(e.value)
    wide = m.Index(33, 1024)                                         # k = 33
    with pytest.raises(m.MfxError) as e:
        m.Binner(m.Evaluator(wide, m.KParams(1.0)))
    assert e.value.code == -1 and "k <= 31" in str(e.value)
    sx = m.Index(k, len(ra[0]) + 16)                                 # a sharded index
    sx.set_shard(0, 2)
    sx.add_read(*ra)
    with pytest.raises(m.MfxError) as e:
        m.Binner(m.Evaluator(sx, m.KParams(1.0)))
    assert e.value.code == -1 and "shard" in str(e.value)
    # a record of 2^32 bases: refused before a base is read, nothing of the call is taken
    b = m.Binner(ev, 100)
    ptrs = (C.c_char_p * 2)(b"ACGT" * 10, b"ACGT")
    lens = (C.c_uint64 * 2)(40, 2**32)
    assert L.mfx_bin_add(b.h, ptrs, lens, 2) == -1 and b"2^32" in L.mfx_last_error()
    assert L.mfx_bin_add(b.h, None, lens, 2) == -1
    b.add([b"ACGT" * 10])
    b.flush()
    assert b.ready() == 1 and b.take(5)[:, 0].tolist() == [40 - k + 1]
    st = b.end()
    assert st["reads"] == 1 and st["bases"] == 40
