"""mfx_dump_values / mfx_dump_values_sharded over the range grid of tests/dump_ranges.py, once per route to a value:
mfx_dump_kernel<CANON, RECOUNT, COMPACT> in the four instances -dump can reach, mfx_w_dump_kernel<CANON>, a sequence that
holds only its packed planes, the sharded sum and recount.  Every answer -- both arrays, both counters -- is compared exactly with the
oracles' (merfin-dump.C:44-67); the ranges begin on tile boundaries and inside tiles, right behind Ns, end inside the last
k - 1 positions of a contig, are empty or hold no k-mer at all (tests/test_dump_ranges_cpu.py shows the grid has them all
and that the checker fails on each slip the range arithmetic could make)."""
import numpy as np
import pytest

from tests import dump_ranges as dr

pytestmark = pytest.mark.gpu
LONG, L = dr.LONG, dr.L_LONG


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _full_index(m, w):
    rk, rv = w.arrays(w.read)
    ak, av = w.arrays(w.asm)
    ix = m.Index(w.k, len(rv) + len(av) + 16)
    ix.add_read(rk, rv)
    ix.add_asm(ak, av)
    return ix


def _kparams(m, ref):
    return m.KParams(ref.peak, ref.probK or None, ref.probP or None)


def _grid(route, ref, fn):
    n = ref.run_grid(fn)
    assert n == dr.grid_size(ref.w)
    print("-dump ranges, %s: %d ranges checked" % (route, n))


@pytest.mark.parametrize("use_prob", [False, True], ids=["peak", "table"])
def test_full_table_canonical_k21(use_prob):
    m = _mfx()
    w = dr.world(21)
    ref = dr.Reference(w, dr.PEAK, *(dr.golden_table() if use_prob else (None, None)))
    ix = _full_index(m, w)
    assert ix.info()["canonical"] and not ix.info()["compact"]
    ev, seqs = m.Evaluator(ix, _kparams(m, ref)), m.Sequences(w.contigs)
    _grid("full table, canonical, k = 21, %s" % ("golden table" if use_prob else "peak rule"), ref, lambda c, b, e: ev.dump_values(seqs, c, b, e))


def test_full_table_even_k_doubles_its_palindromes():
    m = _mfx()
    w = dr.world(20)
    ref = dr.Reference(w)
    ix = _full_index(m, w)
    assert ix.info()["canonical"]
    ev, seqs = m.Evaluator(ix, _kparams(m, ref)), m.Sequences(w.contigs)
    _grid("full table, k = 20", ref, lambda c, b, e: ev.dump_values(seqs, c, b, e))


def test_non_canonical_database_both_strands():
    m = _mfx()
    w = dr.world(21, False)
    ref = dr.Reference(w, dr.PEAK, *dr.golden_table())
    ix = _full_index(m, w)
    assert not ix.info()["canonical"]
    ev, seqs = m.Evaluator(ix, _kparams(m, ref)), m.Sequences(w.contigs)
    _grid("full table, forward k-mers, k = 21", ref, lambda c, b, e: ev.dump_values(seqs, c, b, e))


def test_canonical_database_under_forced_two_strand(monkeypatch):
    """MFX_FORCE_TWO_STRAND=1 is read by the -hist launcher; -dump decides by the database alone, and its answers for the
    canonical world must not move under the knob"""
    m = _mfx()
    w = dr.world(21)
    ref = dr.Reference(w)
    monkeypatch.setenv("MFX_FORCE_TWO_STRAND", "1")
    ix = _full_index(m, w)
    ev, seqs = m.Evaluator(ix, _kparams(m, ref)), m.Sequences(w.contigs)
    _grid("full table, canonical, MFX_FORCE_TWO_STRAND=1", ref, lambda c, b, e: ev.dump_values(seqs, c, b, e))


@pytest.mark.parametrize("load_factor", [None, "0.9"], ids=["lf-default", "lf-0.9"])
def test_compact_sequence_only_index(load_factor, tmp_path, monkeypatch):
    """Index.for_seq + build_for_hist: 8-byte slots, the counts beyond the slot's fields (60000, 2**22 - 1, 2**32 - 1) in the side
    table, read k-mers that are in no contig dropped.  (A sequence-only index refuses a database of forward k-mers, so the
    COMPACT instance that probes both strands is out of -dump's reach.)"""
    m = _mfx()
    if load_factor:
        monkeypatch.setenv("MFX_LOAD_FACTOR", load_factor)
    w = dr.world(21)
    ref = dr.Reference(w, dr.PEAK, *dr.golden_table())
    db = str(tmp_path / "read.mfxk")
    m.db_write_flat(db, w.k, *w.arrays(w.read))
    seqs = m.Sequences(w.contigs)
    ix = m.Index.for_seq(w.k, sum(len(c) for c in w.contigs) + 16)
    ix.build_for_hist(seqs, db)
    info = ix.info()
    assert info["seq_only"] and info["compact"] and info["canonical"] and info["distinct"] == len(w.asm)
    assert info["dropped"] == sum(1 for x in w.read if x not in w.asm) > 100
    ev = m.Evaluator(ix, _kparams(m, ref))
    assert max(dr.SPECIAL) == 2**32 - 1 and all(int(ref.rv[ci][p]) == v for v in dr.SPECIAL[-3:] for ci, p in w.placed[v])
    _grid("compact sequence-only index, load factor %s" % (load_factor or "default"), ref, lambda c, b, e: ev.dump_values(seqs, c, b, e))


@pytest.mark.parametrize("canonical", [True, False], ids=["canonical", "forward"])
@pytest.mark.parametrize("k", [33, 64])
def test_wide_kmers(k, canonical):
    """mfx_w_dump_kernel against oracle.plain"""
    m = _mfx()
    w = dr.world(k, canonical)
    ref = dr.Reference(w)
    ix = _full_index(m, w)
    assert bool(ix.info()["canonical"]) == canonical and ix.info()["k"] == k
    ev, seqs = m.Evaluator(ix, _kparams(m, ref)), m.Sequences(w.contigs)
    _grid("128-bit k-mers, k = %d, %s" % (k, "canonical" if canonical else "forward k-mers"), ref, lambda c, b, e: ev.dump_values(seqs, c, b, e))


def test_sequence_that_holds_only_its_packed_planes(monkeypatch):
    """Sequences.create + a streamed -hist, or a packed upload, leave the 2-bit planes only; the first -dump call makes one byte
    per base from them (mfx_seq_ensure_ascii).  That first call is a range of its own kind each time; the grid follows on a
    sequence that has been unpacked"""
    import time
    m = _mfx()
    w = dr.world(21)
    ref = dr.Reference(w)
    ev = m.Evaluator(_full_index(m, w), _kparams(m, ref))
    k, lens = w.k, [len(c) for c in w.contigs]
    kasm = sum(ref.counters(ci, 0, n)[0] for ci, n in enumerate(lens))
    monkeypatch.setenv("MFX_UPLOAD_PACKED_MIN", "1")                   # the packed transport for an upload of any size
    firsts = [(LONG, 4097, 4096 + k), (LONG, 8193, L), (LONG, 4096, 8192), (LONG, 257, 4095), (LONG, L - k + 1, L), (LONG, 0, 0),
              (8, 4096, 4096 + k - 1), (2, 0, k), (LONG, 0, L)]
    for i, (c, b, e) in enumerate(firsts):
        assert (b, e) in dr.grid(w, c)
        t0 = time.time()
        if i < 2:
            seqs = m.Sequences.create(lens)
            assert ev.hist_streamed(seqs, w.contigs).kasm == kasm
        else:
            seqs = m.Sequences(w.contigs)
        print("packed-only sequence %d made in %.2f s" % (i, time.time() - t0))
        assert seqs.packed
        ref.check(ev.dump_values(seqs, c, b, e), c, b, e)              # the call that unpacks
        ref.check(ev.dump_values(seqs, c, b, e), c, b, e)              # ... and the same range after it
    _grid("packed planes unpacked on first use", ref, lambda c, b, e: ev.dump_values(seqs, c, b, e))


@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_sum_and_recount(shards):
    """mfx_dump_values_sharded: every shard answers for its k-mers, the arrays are added, and the RECOUNT instance takes both
    counters from the sums -- under the golden table, where a non-zero count can be missing"""
    m = _mfx()
    from tests.test_gpu_sharded import _build_shards
    w = dr.world(21)
    ref = dr.Reference(w, dr.PEAK, *dr.golden_table())
    ixs = _build_shards(m, w.k, w.arrays(w.read), w.arrays(w.asm), shards)
    assert all(ix.info()["distinct"] > 0 for ix in ixs)
    evs = [m.Evaluator(ix, _kparams(m, ref)) for ix in ixs]
    seqs = m.Sequences(w.contigs)
    _grid("sharded, %d shards on one device, golden table" % shards, ref, lambda c, b, e: m.dump_values_sharded(evs, [seqs] * shards, c, b, e))


def test_refusals_leave_the_evaluator_answering():
    m = _mfx()
    from merfin_amd import binding
    from tests.test_gpu_sharded import _build_shards
    w = dr.world(21)
    ref = dr.Reference(w)
    seqs = m.Sequences(w.contigs)
    ev = m.Evaluator(_full_index(m, w), _kparams(m, ref))
    evs = [m.Evaluator(ix, _kparams(m, ref)) for ix in _build_shards(m, w.k, w.arrays(w.read), w.arrays(w.asm), 2)]
    wide = dr.world(33)
    wref = dr.Reference(wide)
    wseqs = m.Sequences(wide.contigs)
    wev = m.Evaluator(_full_index(m, wide), _kparams(m, wref))
    routes = [(ref, lambda c, b, e: ev.dump_values(seqs, c, b, e)),
              (ref, lambda c, b, e: m.dump_values_sharded(evs, [seqs, seqs], c, b, e)),
              (wref, lambda c, b, e: wev.dump_values(wseqs, c, b, e))]
    good = (LONG, 4097, 8193)
    for rf, fn in routes:
        for bad in ((LONG, 4097, 4096), (LONG, L, 0), (LONG, 0, L + 1), (LONG, L + 1, L + 1), (4, 0, 4096), (len(w.contigs), 0, 0), (2**32 - 1, 0, 0)):
            with pytest.raises(m.MfxError) as err:
                fn(*bad)
            assert binding.MFX_ERRORS[err.value.code] == "INVAL", (bad, str(err.value))
            rf.check(fn(*good), *good)
    assert np.array_equal(ev.dump_values(seqs, LONG, 0, L)[0], ref.rv[LONG])
