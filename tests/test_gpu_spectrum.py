"""Index.spectrum (mfx_spectrum_kernel, mfx_w_spectrum_kernel) against the reference image of tests/spectrum_ref.py on every
table form.  The expected side comes from the (k-mer, count) tables alone; every comparison is `==` on integers; every image is
taken twice with equal bytes and sums to the entry count the call reports."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import kstar_grid as kg
from tests import spectrum_ref as sr
from tests import synth
from tests import synth_reads
from tests.test_gpu_parity import build_index
from tests.test_gpu_seqonly import seq_index
from tests.test_gpu_wide import to_rows

pytestmark = pytest.mark.gpu

E_INVAL = -1
EXTRA = (2046, 2047, 2048, 65535, 2 ** 31, 2 ** 32 - 1)
COPIES = (1, 4, 6)
MAX_MULT = (4, 16, 1023, 1024, 1025, 2048, 5000, 65536)
_worlds = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _spectrum(ix, copies, max_mult):
    """the image, taken twice: equal bytes, and its sum is the entry count"""
    a, na = ix.spectrum(copies, max_mult, with_entries=True)
    b, nb = ix.spectrum(copies, max_mult, with_entries=True)
    assert a.shape == (copies + 2, max_mult + 1) and a.dtype == np.uint64
    assert a.tobytes() == b.tobytes() and na == nb == int(a.sum(dtype=np.uint64))
    return a, na


def grid_pairs():
    """every (readV, asmV) of [0, 2100] x [0, 9] but (0, 0) -- whatever number of columns below 2048 the kernel keeps in LDS, both
    sides of that boundary are occupied in every row, and so is the overflow column -- plus the counts around the 11-bit fields
    and the ends of uint32 on both sides"""
    S = {(r, a) for r in range(2101) for a in range(10)} - {(0, 0)}
    S.update((e, a) for e in EXTRA for a in range(10))
    S.update((r, e) for r in (0, 1, 5, 1023, 1024, 2046, 2047, 2048) for e in EXTRA)
    S.update((e, f) for e in EXTRA for f in EXTRA)
    return sorted(S)


def grid_world(k):
    """one world per k (tests/kstar_grid.py assigns the pairs to the canonical k-mers of a small assembly); shared, unchanged"""
    if k not in _worlds:
        pairs = grid_pairs()
        w = kg.build_world(k, pairs, set(pairs), seed=40 + k, palindromes=8 if k % 2 == 0 else 0)
        assert set(w.pair_of.values()) == set(pairs)
        v = np.array(list(w.pair_of.values()), dtype=np.uint64)
        w.rv, w.av = v[:, 0].copy(), v[:, 1].copy()
        _worlds[k] = w
    return _worlds[k]


def _check_grid(ix, w, minV=0, maxV=2 ** 64 - 1, copies=COPIES, max_mult=MAX_MULT):
    for c in copies:
        for mm in max_mult:
            want = sr.image_of_pairs(w.rv, w.av, c, mm, minV, maxV)
            got, n = _spectrum(ix, c, mm)
            np.testing.assert_array_equal(got, want, err_msg="copies %d max_mult %d" % (c, mm))
            assert n == int(want.sum(dtype=np.uint64))
            if minV == 0 and maxV >= 2 ** 32 - 1:                  # the case is what it claims to be: every column up to 2100 and the overflow column, in every row
                assert want[:, 1:min(mm, 2100) + 1].all() and want[:, mm].all()


@pytest.mark.parametrize("k", [15, 21, 22, 31])
def test_grid_full_table(k):
    m = _mfx()
    w = grid_world(k)
    if k % 2 == 0:
        assert w.n_pal >= 4
    read, asm = kg.tables(w)
    ix = build_index(m, k, read, asm)
    assert ix.info()["canonical"] and not ix.info()["seq_only"]
    _check_grid(ix, w)


@pytest.mark.parametrize("k", [19, 21, 25, 31])
def test_grid_sequence_only_compact_and_quotient(k):
    """k <= 21: the k-mer in the slot; above: its quotient.  Every k-mer of the world is a k-mer of the sequence, so the table holds
    them all -- those absent from the assembly table with assembly count 0"""
    m = _mfx()
    w = grid_world(k)
    read, asm = kg.tables(w)
    ix, _ = seq_index(m, k, w.contigs, read, asm)
    assert ix.info()["compact"] and ix.info()["seq_only"] and ix.info()["distinct"] == len(w.keys)
    _check_grid(ix, w)


@pytest.mark.parametrize("k", [33, 64])
def test_grid_wide(k):
    m = _mfx()
    w = grid_world(k)
    read, asm = kg.tables(w)
    ix = m.Index(k, len(read[0]) + len(asm[0]) + 16)
    ix.add_read(to_rows(read[0]), read[1])
    ix.add_asm(to_rows(asm[0]), asm[1])
    _check_grid(ix, w)


@pytest.mark.parametrize("k,lf,seed", [(22, "0.5", 1), (22, "0.85", 2), (24, "0.85", 5)])
def test_crowded_quotient_tables(k, lf, seed, monkeypatch):
    """the worlds of test_quotient_form_crowded_tables_and_the_side_table: k-mers beyond their three candidate lines (they live in
    the side table only) next to saturated fields (whose exact counts live there too) -- each counted once"""
    import torch
    from merfin_amd.distributed import _DeviceBytes
    m = _mfx()
    monkeypatch.setenv("MFX_LOAD_FACTOR", lf)
    r = np.random.default_rng(9000 + seed)
    peak = float(r.choice([2.5, 9.0, 26.0]))
    contigs, read, asm = synth.world(k=k, peak=peak, seed=9100 + seed, sizes=(60000, 20000, 4097, 30, 0), err_kmers=1500)
    rv = read[1].astype(np.uint64)
    big = r.random(len(rv)) < 0.03
    rv[big] = r.choice([2046, 2047, 2048, 5000, 200000], size=int(big.sum()))
    read = (read[0], rv.astype(np.uint32))
    seqs = m.Sequences(contigs)
    ix = m.Index.for_seq(k, sum(len(c) for c in contigs) + 16)
    ix.count_asm(seqs)
    for part in (read[1] // 2, read[1] - read[1] // 2):
        ix.add_read(read[0], part)
    info = ix.info()
    assert info["compact"] and info["distinct"] == len(asm[0])
    # both occur, or the case proves nothing: saturated fields (the export's raw counts), and k-mers that have no slot in the main
    # lines (8-byte slots, all ones = empty; the main lines come first in the image)
    _, er, ea = ix.export()
    assert int(((er >= 2047) | (ea >= 2047)).sum()) > 100
    lines, nbytes, _, _ = ix.device_image()
    main = torch.as_tensor(_DeviceBytes(lines, nbytes), device="cuda")[:info["capacity"] * 8].view(torch.int64)
    beyond = info["distinct"] - int((main != -1).sum().item())
    print("k %d load factor %s: %d k-mers, %d beyond their candidate lines" % (k, lf, info["distinct"], beyond))
    assert beyond > 0
    for c, mm in ((4, 10000), (1, 1024), (6, 65536)):
        want = sr.image(read, asm, c, mm, seq_only=True)
        got, n = _spectrum(ix, c, mm)
        np.testing.assert_array_equal(got, want)
        assert n == len(asm[0])


@pytest.mark.parametrize("form", ["full", "compact"])
def test_read_filter(form):
    """-min 2 -max 2500: outside it the read count is 0, and a read-only k-mer filtered to (0, 0) is no entry any more"""
    m = _mfx()
    k, lo, hi = 21, 2, 2500
    w = grid_world(k)
    read, asm = kg.tables(w)
    ix = build_index(m, k, read, asm, lo, hi) if form == "full" else seq_index(m, k, w.contigs, read, asm, lo, hi)[0]
    assert ix.info()["compact"] == (form == "compact")
    gone = int((((w.rv < lo) | (w.rv > hi)) & (w.av == 0)).sum())
    assert gone >= 4
    _check_grid(ix, w, lo, hi, copies=(4,), max_mult=(1024, 5000))
    assert _spectrum(ix, 4, 5000)[1] == len(w.keys) - gone


def test_table_larger_than_one_grid_pass():
    """a ~64 MB table, almost all of it empty: several turns of every block's loop, and the empty-slot skip"""
    m = _mfx()
    k = 21
    _, read, asm = synth.world(k=k, seed=61)
    ix = build_index(m, k, read, asm, cap=4000000)
    assert ix.info()["bytes"] >= 60e6
    for c, mm in ((4, 10000), (2, 16)):
        want = sr.image(read, asm, c, mm)
        got, n = _spectrum(ix, c, mm)
        np.testing.assert_array_equal(got, want)
        assert n == len(np.union1d(read[0], asm[0]))


def test_smallest_tables():
    m = _mfx()
    for k in (21, 25, 33):
        contig = synth.random_contig(synth.rng(k), k).tobytes()
        seqs = m.Sequences([contig])
        if k <= 31:
            ix = m.Index.for_seq(k, 64)
            ix.count_asm(seqs)
        else:
            ix = m.Index(k, 64)
            ix.count_asm(seqs)
        want = np.zeros((6, 101), dtype=np.uint64)
        want[1, 0] = 1                                             # one k-mer, once in the assembly, no reads
        got, n = _spectrum(ix, 4, 100)
        np.testing.assert_array_equal(got, want)
        assert n == 1
    # no entry at all: the full table, the two sequence-only forms before any claim, 32 <= k
    for ix in (m.Index(21, 1000), m.Index.for_seq(21, 1000), m.Index.for_seq(25, 1000), m.Index(40, 1000)):
        got, n = _spectrum(ix, 4, 100)
        assert n == 0 and not got.any()
        got, n = _spectrum(ix, 6, 65536)
        assert n == 0 and not got.any()


@pytest.mark.parametrize("k", [21, 31])
def test_read_counted_index(k):
    """Index.count_reads: the spectrum of the counted reads over the assembly's k-mers"""
    m = _mfx()
    asm, reads = synth_reads.reads_world(k, 700 + k)
    ak, av = po.count_kmers(k, asm)
    rk, rv = po.count_kmers(k, reads)
    seqs = m.Sequences(asm)
    ix = m.Index.for_seq(k, sum(len(c) for c in asm) + 16)
    ix.count_asm(seqs)
    ix.count_reads(reads)
    for c, mm in ((4, 10000), (3, 8)):
        want = sr.image((rk, rv), (ak, av), c, mm, seq_only=True)
        got, n = _spectrum(ix, c, mm)
        np.testing.assert_array_equal(got, want)
        assert n == len(ak)


def test_three_shards_add_up():
    m = _mfx()
    k, n = 21, 3
    w = grid_world(k)
    read, asm = kg.tables(w)
    total, entries = np.zeros((6, 5001), dtype=np.uint64), []
    for r in range(n):
        ix = m.Index(k, len(read[0]) + len(asm[0]) + 16)
        ix.set_shard(r, n)
        ix.add_read(*read)
        ix.add_asm(*asm)
        got, cnt = _spectrum(ix, 4, 5000)
        total += got
        entries.append(cnt)
    assert min(entries) > len(w.keys) // 6 and sum(entries) == len(w.keys)
    np.testing.assert_array_equal(total, sr.image_of_pairs(w.rv, w.av, 4, 5000))


def test_forward_strand_database_is_refused():
    """a database of forward-strand k-mers splits a k-mer over two entries: no spectrum of k-mers"""
    m = _mfx()
    k = 11
    c = synth.random_contig(synth.rng(11), 3000).tobytes()
    _, _, f, rc = kg.contig_kmers(c, k)
    fwd = np.array(sorted({a for a, b in zip(f, rc) if a > b}), dtype=np.uint64)
    assert len(fwd) > 500
    ix = m.Index(k, 2 * len(fwd) + 16)
    ix.add_read(fwd, np.full(len(fwd), 7, dtype=np.uint32))
    assert not ix.info()["canonical"]
    with pytest.raises(m.MfxError) as e:
        ix.spectrum(4, 100)
    assert e.value.code == E_INVAL and "non-canonical" in str(e.value)
    # ... as are arguments out of range, on any index
    ok = m.Index(21, 100)
    for c_, mm in ((0, 100), (7, 100), (4, 3), (4, 65537)):
        with pytest.raises(m.MfxError) as e:
            ok.spectrum(c_, mm)
        assert e.value.code == E_INVAL and "outside" in str(e.value)


def _canonical(x, k):
    """canonical form of 2-bit coded k-mers (A 0, C 1, T 2, G 3: the complement is code ^ 2), k <= 31"""
    x = np.asarray(x, dtype=np.uint64)
    rc, y = np.zeros_like(x), x.copy()
    for _ in range(k):
        rc = (rc << np.uint64(2)) | ((y & np.uint64(3)) ^ np.uint64(2))
        y >>= np.uint64(2)
    return np.minimum(x, rc)


@pytest.mark.parametrize("agg", ["0", "1"])
@pytest.mark.parametrize("shape", ["skewed", "flat"])
def test_skewed_and_flat_shapes(shape, agg, monkeypatch):
    """skewed: 200 000 entries, 90 % of them read-only k-mers seen once (one LDS bin for whole waves: the fast path of the
    wave-aggregated form), the others one cell each; flat: every entry a different cell.  Both forms of the kernel (MFX_SPECTRUM_AGG)"""
    m = _mfx()
    monkeypatch.setenv("MFX_SPECTRUM_AGG", agg)
    k = 21
    r = np.random.default_rng(77)
    cells = np.array([(rv, av) for rv in range(1, 3001) for av in range(7)], dtype=np.uint64)      # 21 000 distinct cells
    n = 200000 if shape == "skewed" else len(cells)
    keys = np.unique(_canonical(r.integers(0, 4 ** k, size=n + n // 8, dtype=np.uint64), k))
    keys = keys[r.permutation(len(keys))[:n]]
    assert len(keys) == n
    rv, av = np.ones(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    m_ = 20000 if shape == "skewed" else n
    rv[:m_], av[:m_] = cells[:m_, 0], cells[:m_, 1]
    ix = m.Index(k, n + 16)
    ix.add_read(keys, rv.astype(np.uint32))
    ix.add_asm(keys[av > 0], av[av > 0].astype(np.uint32))
    want = sr.image_of_pairs(rv, av, 6, 5000)
    assert int(want.max()) == (n - m_ + 1 if shape == "skewed" else 1)
    got, cnt = _spectrum(ix, 6, 5000)
    np.testing.assert_array_equal(got, want)
    assert cnt == n
