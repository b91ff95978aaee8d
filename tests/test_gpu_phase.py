"""Evaluator.phase / mfx_phase_run: hap-mer markers of two sets, their runs and phase blocks, made on the device.  The expected records
are the membership of every position's canonical k-mer in the two sets (np.isin on per-position canonical k-mers that are checked
against the oracle's count of the assembly; the plain-Python restatement oracle/plain.py for 32 <= k <= 64) taken through the
sequential walk of tests/phase_ref.py.  The sets are taken from planned positions of the contigs so that the plane shapes of
tests/test_phase_cpu.py occur in the real planes.  EVERY field of EVERY record is compared with `==`."""
import gzip

import numpy as np
import pytest

from oracle import plain
from oracle import pyoracle as po
from tests import phase_ref as pr
from tests import synth
from tests import track_ref as tr
from tests.test_gpu_parity import build_index
from tests.test_gpu_seqonly import seq_index
from tests.test_gpu_wide import small_world, build as build_wide

pytestmark = pytest.mark.gpu

SIZES = (120000, 9000, 4096, 4097, 500, 20, 10, 0, 8191)       # > 100 000, shorter than k, empty, one position past a tile
SWITCHES = (0, 1, 3, 100)
A, B = 0, 1
SEEDS = {15: 8015, 21: 8021, 22: 8122, 31: 8031}               # worlds whose planned edge positions all hold a valid k-mer


def ranges_of(k):
    return (0, k, 64, 5000, 10**6)


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def kmers_of(k, contig):
    """(valid, forward, reverse-complement) k-mer of every start position, k <= 31 (2 bits a base: (c >> 1) & 3, first base highest)"""
    b = np.frombuffer(contig, dtype=np.uint8)
    code = ((b >> 1) & 3).astype(np.uint64)
    n = len(b)
    valid = tr.valid_starts(contig, k)
    f, r = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    m = n - k + 1
    if m > 0:
        for i in range(k):
            f[:m] = (f[:m] << np.uint64(2)) | code[i:i + m]
            r[:m] |= (code[i:i + m] ^ np.uint64(2)) << np.uint64(2 * i)
    return valid, f, r


class World:
    """contigs; per contig the valid mask and the canonical k-mer of every position (uint64, or Python integers for k > 31); the
    occurrences of every canonical k-mer in the whole assembly"""

    def __init__(self, k, contigs, valid, canon, unique=True):
        self.k, self.contigs, self.valid, self.canon = k, contigs, valid, canon
        self.count = {}
        for v, c in zip(valid, canon):
            for x in np.asarray(c, dtype=object)[v].tolist():
                self.count[x] = self.count.get(x, 0) + 1
        # unique: markers are planned only where the k-mer occurs once, so that it flags no other place
        self.usable = [v & np.array([self.count.get(x, 0) == 1 for x in np.asarray(c, dtype=object).tolist()], dtype=bool) if unique and len(v) else v
                       for v, c in zip(valid, canon)]
        self.marks, self.taken = [], set()

    def edge(self, c, p, h, unique=True):
        """a marker at exactly this position (unique=False: its k-mer may occur elsewhere and flag that place too)"""
        assert (self.usable[c][p] if unique else self.valid[c][p]) and (c, p) not in self.taken, (c, p)
        self.taken.add((c, p))
        self.marks.append((c, p, h))

    def bulk(self, c, p, n, h, step=5):
        """n markers of one haplotype from p on, about `step` apart, on positions whose k-mer occurs once -> the position behind them"""
        while n:
            if self.usable[c][p] and (c, p) not in self.taken:
                self.edge(c, p, h)
                n -= 1
            p += step
        return p

    def sets(self, shared=(), foreign=()):
        """the two sets as sorted lists of canonical k-mers: the planned markers, k-mers in both, k-mers that occur nowhere"""
        a = {self.canon[c][p] for c, p, h in self.marks if h == A} | {self.canon[c][p] for c, p in shared} | set(foreign[0::2])
        b = {self.canon[c][p] for c, p, h in self.marks if h == B} | {self.canon[c][p] for c, p in shared} | set(foreign[1::2])
        return sorted(int(x) for x in a), sorted(int(x) for x in b)

    def masks(self, a, b):
        """per contig (in A and not in B, in B and not in A, in both, valid) by membership of the position's canonical k-mer"""
        out = []
        wide = self.k > 31
        sa, sb = set(a), set(b)
        for v, c in zip(self.valid, self.canon):
            if wide:
                ina = np.array([x in sa for x in c], dtype=bool)
                inb = np.array([x in sb for x in c], dtype=bool)
            else:
                ina, inb = np.isin(c, np.array(a, dtype=np.uint64)), np.isin(c, np.array(b, dtype=np.uint64))
            ina, inb = ina & v, inb & v
            out.append((ina & ~inb, inb & ~ina, ina & inb, v))
        return out


def narrow_world(k, seed):
    contigs, _, asm = synth.world(k=k, peak=17.3, seed=seed, sizes=SIZES, err_kmers=0)
    c0 = bytearray(contigs[0])
    c0[70000:70300] = c0[60000:60300]                          # a duplicated 300-base segment: one marker k-mer flags two places
    contigs[0] = bytes(c0)
    valid, canon = [], []
    for c in contigs:
        v, f, r = kmers_of(k, c)
        valid.append(v)
        canon.append(np.minimum(f, r))
    # the per-position canonical k-mers are the oracle's: their multiset is its count of the assembly
    ok, oc = po.count_kmers(k, contigs)
    mk, mc = np.unique(np.concatenate([c[v] for c, v in zip(canon, valid)]), return_counts=True)
    assert np.array_equal(mk, ok) and np.array_equal(mc.astype(np.uint64), oc.astype(np.uint64))
    return World(k, contigs, valid, canon)


def n_run(contig):
    """[n0, n1): the 200-N run of synth.decorate"""
    isn = np.flatnonzero((np.frombuffer(contig, dtype=np.uint8) & 0xDF) == ord("N"))
    run = max(np.split(isn, np.flatnonzero(np.diff(isn) != 1) + 1), key=len)
    assert len(run) >= 200
    return int(run[0]), int(run[-1]) + 1


def plan_shapes(w):
    """the shapes of tests/test_phase_cpu.py at planned positions of the SIZES world -> the positions of the shared k-mers"""
    k, T = w.k, 4096
    # bits 63 | 0 of adjacent words, positions 4095 | 4096, same and opposite haplotypes over the edge
    for p, h in ((60, A), (63, A), (64, B), (127, B), (128, B), (191, A), (192, A), (4095, A), (4096, A), (8191, A), (8192, B)):
        w.edge(0, p, h)
    # a run continued across 3 empty tiles (5, 6, 7), two runs of opposite haplotypes separated by 3 empty tiles (9, 10, 11)
    w.bulk(0, 4 * T + 4000, 1, A, step=1)
    w.bulk(0, 8 * T + 7, 1, A, step=1)
    w.bulk(0, 8 * T + 100, 1, B, step=1)
    w.bulk(0, 12 * T + 3, 1, A, step=1)
    # long runs with intrusions of 3, 4, 100 and 101 markers; 200 alternating markers; short runs in front of and behind long ones
    p = w.bulk(0, 13 * T + 10, 1, B)
    p = w.bulk(0, p, 150, A)
    for n in (3, 4, 100, 101):
        p = w.bulk(0, p, n, B)
        p = w.bulk(0, p, 150, A)
    p = w.bulk(0, p, 1, B)
    p = 80000
    for i in range(200):
        p = w.bulk(0, p, 1, i & 1, step=7)
    # a long A run, short B and A runs, a B run spread over more than 5000 bases
    p = w.bulk(0, 90000, 120, A)
    p = w.bulk(0, p, 1, B)
    p = w.bulk(0, p, 1, A)
    p = w.bulk(0, p, 50, B, step=120)                          # n <= 100 and span > 5000: long by its span at (100, 5000)
    # the duplicated segment: one k-mer, two markers
    w.taken.add((0, 70100))
    w.marks.append((0, 60100, B))
    assert w.valid[0][60100] and w.canon[0][60100] == w.canon[0][70100] and w.count[w.canon[0][60100]] == 2
    # the last k-mer of contig 1 and the first of contig 2; both sides of contig 1's N run
    n0, n1 = n_run(w.contigs[1])
    for c, p, h in ((1, n0 - k - 3, A), (1, n0 - k, A), (1, n1, B), (1, n1 + 2, B), (1, len(w.contigs[1]) - k, A), (2, 0, A), (2, 4096 - k, B)):
        w.edge(c, p, h, unique=False)
    w.edge(3, 4097 - k, B, unique=False)                                   # a contig of one tile + one position: its second tile holds no k-mer
    # only short runs (S >= 1): a majority on contig 8, a tie on contig 4
    p = 100
    for i in range(5):
        p = w.bulk(8, p, 1, 1 - (i & 1), step=40)
    p = w.bulk(4, 50, 1, B)
    p = w.bulk(4, p + 30, 1, A)
    shared = []
    p = 50000
    while len(shared) < 6:                                    # k-mers of both sets: counted, in no plane; some between markers
        if w.usable[0][p] and (0, p) not in w.taken:
            shared.append((0, p))
        p += 11
    for q in (13 * 4096 + 200, 90100):
        while not (w.usable[0][q] and (0, q) not in w.taken):
            q += 1
        shared.append((0, q))
    return shared


def foreign_kmers(w, n=40):
    """canonical k-mers that occur nowhere in the assembly"""
    r = np.random.default_rng(5)
    out = []
    while len(out) < n:
        s = "".join(r.choice(list("ACGT"), size=w.k))
        x = min(plain.enc(s), plain.enc(plain.revcomp(s)))
        if x not in w.count:
            out.append(x)
    return out


def expected(w, masks, S, R):
    return pr.blocks([pr.markers_of_masks(m[0], m[1]) for m in masks], w.k, S, R)


def counts_of(masks):
    return np.array([[int(v.sum()), int(a.sum()), int(b.sum()), int(s.sum())] for a, b, s, v in masks], dtype=np.uint64).reshape(-1, 4)


def check(m, ev, seqs, w, masks, switches=SWITCHES, ranges=None):
    """the whole grid: records == the reference's; contig_counts == numpy's; every marker is in one block; a second run is byte-identical.
    Returns {(S, R): the records' bytes}"""
    want_counts = counts_of(masks)
    out = {}
    for S in switches:
        for R in (ranges or ranges_of(w.k)):
            got, cc = ev.phase(seqs, S, R)
            assert got.dtype == m.PHASE_DTYPE and got.dtype.itemsize == 48 and cc.dtype == np.uint64 and cc.shape == (len(w.contigs), 4)
            recs = pr.device_records(got)
            assert recs == expected(w, masks, S, R), (S, R)
            assert np.array_equal(cc, want_counts), (S, R)
            for c in range(len(w.contigs)):
                assert sum(r["n_hap"] + r["n_switch"] for r in recs if r["contig"] == c) == int(cc[c, 1] + cc[c, 2]), (S, R, c)
            again, cc2 = ev.phase(seqs, S, R)
            assert got.tobytes() == again.tobytes() and cc.tobytes() == cc2.tobytes(), (S, R)
            out[(S, R)] = got.tobytes()
    return out


def as_tables(a, b):
    """(k-mers, counts) of the two sets; the counts vary: membership is "value > 0", whatever the value"""
    ak, bk = np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)
    return (ak, (1 + np.arange(len(ak)) % 5).astype(np.uint32)), (bk, (1 + np.arange(len(bk)) % 7).astype(np.uint32))


@pytest.mark.parametrize("k", [15, 21, 22, 31])
def test_phase_blocks_match_the_walk(k):
    m = _mfx()
    w = narrow_world(k, SEEDS[k])
    shared = plan_shapes(w)
    a, b = w.sets(shared, foreign_kmers(w))
    masks = w.masks(a, b)
    # the planned shapes are in the expected planes
    T = 4096
    mk0 = masks[0][0] | masks[0][1]
    assert mk0[4095] and mk0[4096] and mk0[63] and mk0[64] and masks[0][0][63] and masks[0][1][64]
    assert not mk0[5 * T:8 * T].any() and not mk0[9 * T:12 * T].any() and mk0[4 * T:5 * T].any() and mk0[8 * T:9 * T].any() and mk0[12 * T:13 * T].any()
    assert masks[0][1][60100] and masks[0][1][70100]          # one k-mer, two markers
    assert masks[1][0][len(w.contigs[1]) - k] and masks[2][0][0]
    assert sum(int(mm[2].sum()) for mm in masks) >= len(shared) and not any((mm[0] & mm[1]).any() for mm in masks)
    assert [int((mm[0] | mm[1]).sum()) for mm in masks][5:8] == [0, 0, 0]       # nothing planned on the shortest contigs
    ra, rb = as_tables(a, b)
    # the compact sequence-only index: the k-mers of the sequence claimed, A and B loaded update-only
    ix, seqs = seq_index(m, k, w.contigs, ra, rb)
    assert ix.info()["seq_only"] and ix.info()["compact"]
    ev = m.Evaluator(ix, m.KParams(17.3))
    base = check(m, ev, seqs, w, masks)
    # every block rule is exercised: blocks of both haplotypes, switch markers inside blocks at S = 3 and S = 100
    for S in (3, 100):
        recs = pr.device_records(np.frombuffer(base[(S, 5000)], dtype=m.PHASE_DTYPE))
        assert {r["hap"] for r in recs} == {A, B} and any(r["n_switch"] for r in recs) and any(r["n_switch_runs"] > 1 for r in recs)
    assert len(base[(0, 0)]) > len(base[(3, 5000)]) > len(base[(100, 5000)]) > 0
    # the records do not depend on the form the sequence is held in, nor on the form of the index
    seqs.pack()
    for (S, R), x in base.items():
        assert ev.phase(seqs, S, R)[0].tobytes() == x, (S, R)
    full = m.Evaluator(build_index(m, k, ra, rb), m.KParams(17.3))
    seqs2 = m.Sequences(w.contigs)
    for (S, R), x in base.items():
        got, cc = full.phase(seqs2, S, R)
        assert got.tobytes() == x and np.array_equal(cc, counts_of(masks)), (S, R)


def test_phase_non_canonical_database():
    """sets of forward-strand k-mers: both strands are probed, a position is in a set when either strand's k-mer is"""
    m = _mfx()
    k = 13
    contigs, _, _ = synth.world(k=k, peak=17.3, seed=8100, sizes=(60000, 2500, 4097, 5, 0), err_kmers=0)
    valid, fw, rc = [], [], []
    for c in contigs:
        v, f, r = kmers_of(k, c)
        valid.append(v); fw.append(f); rc.append(r)
    w = World(k, contigs, valid, [np.minimum(f, r) for f, r in zip(fw, rc)])
    p = w.bulk(0, 100, 1, B)
    for n in (120, 3, 120, 101, 120):
        p = w.bulk(0, p, n, A if n == 120 else B)
    p = w.bulk(0, 4090, 1, A, step=1)
    w.bulk(0, 30000, 40, B, step=9)
    w.bulk(1, 10, 7, A)
    w.bulk(2, 4000, 3, B)
    # the sets hold the k-mers as the sequence spells them; at least one of them is not canonical
    a = np.unique(np.array([fw[c][p] for c, p, h in w.marks if h == A], dtype=np.uint64))
    b = np.unique(np.array([fw[c][p] for c, p, h in w.marks if h == B], dtype=np.uint64))
    assert any(fw[c][p] > rc[c][p] for c, p, h in w.marks)
    masks = []
    for v, f, r in zip(valid, fw, rc):
        ina, inb = (np.isin(f, a) | np.isin(r, a)) & v, (np.isin(f, b) | np.isin(r, b)) & v
        masks.append((ina & ~inb, inb & ~ina, ina & inb, v))
    ix = build_index(m, k, (a, np.ones(len(a), dtype=np.uint32)), (b, np.full(len(b), 3, dtype=np.uint32)))
    assert not ix.info()["canonical"]
    base = check(m, m.Evaluator(ix, m.KParams(5.0)), m.Sequences(contigs), w, masks, switches=(0, 3, 100), ranges=(0, 64, 5000))
    assert len(base[(0, 0)]) > len(base[(100, 5000)]) > 0


@pytest.mark.parametrize("k", [33, 64])
def test_phase_wide_kmers(k):
    m = _mfx()
    contigs, _, _ = small_world(k, 8200 + k)
    valid, canon = [], []
    for c in contigs:
        v = np.zeros(len(c), dtype=bool)
        x = [0] * len(c)
        for i, s in plain.valid_kmers(c, k):
            v[i] = True
            x[i] = min(plain.enc(s), plain.enc(plain.revcomp(s)))
        valid.append(v)
        canon.append(x)
    w = World(k, contigs, valid, canon, unique=False)          # (the contigs of this world repeat each other: a marker k-mer flags several places)
    assert w.count == plain.count_kmers(k, contigs)
    p = w.bulk(0, 5, 1, B)
    for n in (110, 3, 110, 101, 110):
        p = w.bulk(0, p, n, A if n == 110 else B, step=3)
    last = len(contigs[5]) - k
    assert last == 4096
    w.bulk(5, 10, 5, B)
    w.bulk(5, 4070, 25, A, step=1)                            # up to the tile edge of the last contig, and over it
    w.edge(5, 4095, B)
    w.edge(5, last, B)
    shared = []
    q = 6000
    while len(shared) < 3:
        if w.usable[0][q] and (0, q) not in w.taken:
            shared.append((0, q))
        q += 7
    a, b = w.sets(shared, foreign_kmers(w, 10))
    masks = w.masks(a, b)
    assert (masks[5][0] | masks[5][1])[4090:4097].all() and masks[5][1][last] and sum(int(mm[2].sum()) for mm in masks) >= 3
    ix = build_wide(m, k, {x: 1 + i % 5 for i, x in enumerate(a)}, {x: 2 + i % 3 for i, x in enumerate(b)})
    ev = m.Evaluator(ix, m.KParams(9.0))
    base = check(m, ev, m.Sequences([c.encode() for c in contigs]), w, masks, switches=(0, 3, 100), ranges=(0, k, 5000, 10**6))
    assert len(base[(0, 0)]) > len(base[(100, 5000)]) > 0


def test_phase_none_all_refusals_and_text(tmp_path):
    m = _mfx()
    k = 21
    w = narrow_world(k, 8300)
    names = ["c%d" % i for i in range(len(w.contigs))]
    # empty sets: no marker, no block, the valid k-mers counted
    none = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    ix, seqs = seq_index(m, k, w.contigs, none, none)
    ev = m.Evaluator(ix, m.KParams(17.3))
    got, cc = ev.phase(seqs)
    masks = w.masks([], [])
    assert len(got) == 0 and got.dtype == m.PHASE_DTYPE and np.array_equal(cc, counts_of(masks)) and int(cc[:, 0].sum()) > 100000
    m.phase_write(got, cc, seqs, names, k, str(tmp_path / "none"))
    assert (tmp_path / "none.phased_block.bed").read_text() == pr.BED_HEADER
    assert (tmp_path / "none.hapmers.count").read_text() == pr.format_counts(cc.tolist(), names)
    assert (tmp_path / "none.phased_block.stats").read_text() == pr.format_stats([], k, 100, 20000)
    # every k-mer of the assembly in A, every second one in B as well: A markers and shared k-mers only
    allk = np.unique(np.concatenate([c[v] for c, v in zip(w.canon, w.valid)]))
    a, b = allk.tolist(), allk[::2].tolist()
    masks = w.masks(a, b)
    ix, seqs = seq_index(m, k, w.contigs, (allk, np.ones(len(allk), dtype=np.uint32)), (allk[::2], np.ones(len(allk[::2]), dtype=np.uint32)))
    ev = m.Evaluator(ix, m.KParams(17.3))
    base = check(m, ev, seqs, w, masks, switches=(0, 100), ranges=(0, 5000))
    got, cc = ev.phase(seqs, 100, 5000)
    assert int(cc[:, 2].sum()) == 0 and int(cc[:, 3].sum()) > 1000 and set(got["hap"].tolist()) == {A}
    assert len(got) == sum(1 for mm in masks if mm[0].any())  # one block a contig that holds a marker
    # the three texts, plain and compressed, against the formatters
    want = expected(w, masks, 100, 5000)
    for stem, rd in (("all", lambda p: open(p).read()), ("all.gz", lambda p: gzip.open(p, "rt").read())):
        m.phase_write(got, cc, seqs, names, k, str(tmp_path / stem), 100, 5000)
        z = ".gz" if stem.endswith(".gz") else ""
        assert rd(tmp_path / ("all.phased_block.bed" + z)) == pr.format_bed(want, names, k)
        assert rd(tmp_path / ("all.hapmers.count" + z)) == pr.format_counts(counts_of(masks).tolist(), names)
        assert rd(tmp_path / ("all.phased_block.stats" + z)) == pr.format_stats(want, k, 100, 5000)
    bad = got.copy()
    bad["end"][0] = len(w.contigs[0]) + 5                     # a record that is no block of these sequences
    with pytest.raises(m.MfxError):
        m.phase_write(bad, cc, seqs, names, k, str(tmp_path / "x"))
    # a shard of an index cannot answer for membership
    sx = m.Index(k, len(allk) + 16)
    sx.set_shard(0, 2)
    sx.add_read(allk, np.ones(len(allk), dtype=np.uint32))
    with pytest.raises(m.MfxError) as e:
        m.Evaluator(sx, m.KParams(17.3)).phase(m.Sequences(w.contigs))
    assert e.value.code == -1 and "shard" in str(e.value)
