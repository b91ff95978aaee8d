"""Every -hist route of the device against the exact reference of tests/kstar_grid.py, over the exhaustive (readV, asmV) grid:
every tabulated readK / bin / over-copy entry, both sides of every table and bin threshold, and -- with nbins = 1024 -- several
hundred distinct far bins through the open-addressed table.  tests/test_kstar_grid_cpu.py pins the C oracle to the same
reference, so what is compared here is the device and nothing else.

Bars: every integer `==`.  koverCpy against S, the exact rational sum of the reference's double terms:
  * mfx_hist_kernel (+ mfx_hist_rest_kernel) add mfx_kfix(term) -- the term rounded to nearest in units of 2^-52, at most half a
    unit each -- into one integer word per (tile, wave); the words are converted to double (relative 2^-53 each) and summed in a
    fixed order (a tree over W words plus the 64-wide chunk sums: every addition rounds by at most 2^-53 of a partial sum <= S):
        |got - S| <= (n_under + (W + 64) * S) * 2^-53,   W = (MFX_BLOCK / 64) * ntiles.
  * the sharded route (mfx_hist_keys_kernel<true>) TRUNCATES term * 2^52 to an integer -- less than one unit each, all the same
    sign -- into one 128-bit integer, which the host converts once (relative 2^-53; the high word is 0 at these sizes):
        |got - S| <= n_under * 2^-52 + S * 2^-53.
  * mfx_w_hist_kernel (k > 32) sums doubles per lane and block: rel 1e-12, as in test_gpu_wide.py."""
import numpy as np
import pytest

from oracle import plain
from oracle import pyoracle as po
from tests import kstar_grid as kg
from tests import track_ref as tr
from tests.test_gpu_parity import build_index
from tests.test_gpu_seqonly import seq_index
from tests.test_gpu_wide import to_rows
from tests.test_kstar_grid_cpu import CONFIGS, PC, kept_pairs

pytestmark = pytest.mark.gpu

# route -> (k, index kind)
ROUTES = {"k21seq": (21, "seq"), "k31seq": (31, "seq"), "k19seq": (19, "seq"), "k25seq": (25, "seq"), "k22seq": (22, "seq"),
          "k21full": (21, "full"), "k11fwd": (11, "fwd"), "k33wide": (33, "wide"), "k21shard3": (21, "shard")}
WAVES = PC["block"] // 64
_cache = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _world(name, k, kind):
    """one world and its reference per (configuration, k, table form), shared by the routes and tests that use it; unchanged"""
    key = (name, k, kind in ("fwd", "wide") and kind)
    if key not in _cache:
        _, kept = kept_pairs(name)
        pairs = kg.thin(kept, PC["maxp"]) if kind == "wide" else kept
        w = kg.build_world(k, pairs, set(kept), seed=1 + k, canonical=kind != "fwd", palindromes=8 if k % 2 == 0 else 0)
        assert set(w.pair_of.values()) == set(pairs)
        _cache[key] = (w, kg.reference(w, CONFIGS[name], per_position=(k == 21 and kind != "fwd")))
    return _cache[key]


def _kparams(m, cfg):
    _, peak, probK, probP = cfg
    return m.KParams(peak, np.array(probK, dtype=np.uint32) if probK else None, np.array(probP) if probP else None)


def _ntiles(w):
    return sum((len(c) + PC["tile"] - 1) // PC["tile"] for c in w.contigs)


def kover_bound(route_kind, ref, ntiles):
    S = float(ref.S)
    if route_kind == "shard":
        return ref.n_under * 2.0 ** -52 + S * 2.0 ** -53
    return (ref.n_under + (WAVES * ntiles + 64) * S) * 2.0 ** -53


def assert_matches(res, ref, kind, ntiles, what):
    assert (res.kasm, res.kmissing) == (ref.kasm, ref.kmissing), what
    np.testing.assert_array_equal(kg.trim(res.undr()), kg.dense(ref.undr), err_msg=what)
    np.testing.assert_array_equal(kg.trim(res.over()), kg.dense(ref.over), err_msg=what)
    assert res.contig_kasm().tolist() == ref.contig_kasm and res.contig_kmissing().tolist() == ref.contig_kmissing, what
    S = float(ref.S)
    err = abs(float(kg.Fraction(res.koverCpy) - ref.S))
    if kind == "wide":
        print("%s: koverCpy rel err %.3e (bar 1e-12)" % (what, err / S))
        assert res.koverCpy == pytest.approx(S, rel=1e-12)
    else:
        bound = kover_bound(kind, ref, ntiles)
        print("%s: n_under %d S %.6f koverCpy rel err %.3e (bound %.3e)" % (what, ref.n_under, S, err / (S or 1.0), bound / (S or 1.0)))
        assert err <= bound, (what, err, bound)


def far_records(ref, nbins):
    """{key: occurrences} of the bins >= nbins as Evaluator.take_overflow reports them (bit 63: `over`)"""
    want = {i: c for i, c in ref.undr.items() if i >= nbins}
    want.update({(1 << 63) | i: c for i, c in ref.over.items() if i >= nbins})
    return want


def _roomy_side_table(monkeypatch, w):
    """The compact layout keeps counts >= 2047 in a side table sized for 1/64 of the k-mers (never fewer than 8192 slots) and
    refuses the load (MFX_E_FULL) when it fills up.  The ordinary configurations stay below half of that minimum and run on the
    default; a world where most counts are that large asks for a larger table through the knob the library has for it."""
    big = sum(1 for x in w.keys if w.pair_of[x][0] >= PC["field"] or w.pair_of[x][1] >= PC["field"])
    if big > 4096:
        monkeypatch.setenv("MFX_SIDE_DIV", "1")


def _build(m, w, kind, k):
    read, asm = kg.tables(w)
    if kind == "seq":
        ix, seqs = seq_index(m, k, w.contigs, read, asm)
        assert ix.info()["compact"] and ix.info()["seq_only"]
    elif kind == "wide":
        ix = m.Index(k, len(read[0]) + len(asm[0]) + 16)
        ix.add_read(to_rows(read[0]), read[1])
        ix.add_asm(to_rows(asm[0]), asm[1])
        seqs = m.Sequences(w.contigs)
    else:
        ix, seqs = build_index(m, k, read, asm), m.Sequences(w.contigs)
        assert bool(ix.info()["canonical"]) == (kind != "fwd")
    return ix, seqs, read, asm


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_grid_route_matches_exact_reference(name, route, monkeypatch):
    import torch
    m = _mfx()
    k, kind = ROUTES[route]
    cfg = CONFIGS[name]
    w, ref = _world(name, k, kind)
    _roomy_side_table(monkeypatch, w)
    nt = _ntiles(w)
    what = "%s/%s" % (name, route)
    assert ref.n_under > 500 and ref.kmissing > 0
    if k % 2 == 0:
        assert w.n_pal >= 4
    nb_small = PC["nb_lds"]
    far = far_records(ref, nb_small)
    assert len(far) > (100 if kind == "wide" else 300), len(far)
    if kind == "wide":                                           # the plain-Python restatement agrees with the reference on the integers
        ck = plain.count_kmers(k, [c.decode() for c in w.contigs])
        assert sorted(ck) == w.keys
    if kind == "shard":
        n = 3
        read, asm = kg.tables(w)
        ixs = []
        for r in range(n):
            ix = m.Index(k, len(read[0]) + len(asm[0]) + 16)
            ix.set_shard(r, n)
            ix.add_read(*read)
            ix.add_asm(*asm)
            ixs.append(ix)
        seqs = m.Sequences(w.contigs)
        routers = [m.Router(ix, n, min(2, seqs.ntiles)) for ix in ixs]
        for nbins in (0, nb_small):
            evs = [m.Evaluator(ix, _kparams(m, cfg), nbins=nbins) for ix in ixs]
            assert_matches(m.hist_sharded(evs, routers, [seqs] * n), ref, kind, nt, "%s nbins=%d" % (what, nbins))
            assert_matches(m.hist_sharded(evs, routers, [seqs] * n), ref, kind, nt, "%s nbins=%d again" % (what, nbins))
        return
    ix, seqs, read, asm = _build(m, w, kind, k)
    assert seqs.ntiles == nt
    for nbins in (0, nb_small):
        ev = m.Evaluator(ix, _kparams(m, cfg), nbins=nbins)
        assert ev.nbins == (nbins or 65536)
        assert_matches(ev.hist(seqs), ref, kind, nt, "%s nbins=%d" % (what, nbins))
        assert_matches(ev.hist(seqs), ref, kind, nt, "%s nbins=%d again" % (what, nbins))       # the far-bin table was emptied
        if nbins:
            # launch + take_overflow by hand: exactly the far bins, with their occurrence counts
            counts = torch.zeros(m.hist_words(ev.nbins, seqs.ncontigs), dtype=torch.int64, device="cuda")
            kover = torch.zeros(1, dtype=torch.float64, device="cuda")
            assert len(ev.take_overflow()) == 0
            ev.hist_launch(seqs, 0, seqs.ntiles, counts, kover, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            h = counts.cpu().numpy().view(np.uint64)
            rec = ev.take_overflow()
            assert {int(a): int(b) for a, b in rec} == far and len(rec) == len(far), what
            assert int(h[2 * ev.nbins + 2]) == sum(far.values())
            assert_matches(ev.result_from_counts(h, float(kover.item()), seqs.ncontigs).add_overflow(rec), ref, kind, nt, what + " by hand")
            assert len(ev.take_overflow()) == 0
    if route == "k21seq":
        # the same sequence held packed, and uploaded inside the run
        assert_matches(ev.hist_streamed(m.Sequences.create([len(c) for c in w.contigs]), w.contigs), ref, kind, nt, what + " streamed")
        seqs.pack()
        assert_matches(ev.hist(seqs), ref, kind, nt, what + " packed")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_grid_track_matches_reference(name, monkeypatch):
    """-track evaluates K* without the -hist tables (mfx_track.h): the reference's per-position values, reduced per window of
    1000 positions by tests/track_ref.py, `==` every field of every record"""
    m = _mfx()
    k, W = 21, 1000
    w, ref = _world(name, k, "seq")
    _roomy_side_table(monkeypatch, w)
    ix, seqs, _, _ = _build(m, w, "seq", k)
    ev = m.Evaluator(ix, _kparams(m, CONFIGS[name]))
    want = tr.reduce_windows(ref.pp, W)
    rec, kasm, kmissing = ev.track(seqs, W)
    got = tr.device_records(rec)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    assert (kasm, kmissing) == (ref.kasm, ref.kmissing)
    if name != "peak2e-7":                                   # (its candidate set has no k-mer absent from the assembly table)
        assert sum(r["n_nonfinite"] for r in want) > 0       # asmV == 0 with readK > 0


@pytest.mark.parametrize("name", [n for n in CONFIGS if n != "peak2e-7"])
def test_grid_completeness_matches_merge_loop(name):
    """mfx_completeness_kernel has a readK table of its own: its edge and the probK = 0 rows, on the full table"""
    m = _mfx()
    k = 21
    cfg = CONFIGS[name]
    w, ref = _world(name, k, "full")
    ix, seqs, read, asm = _build(m, w, "full", k)
    p = po.Params(k, cfg[1], cfg[2] or None, cfg[3] or None)
    t64, u64 = m.Evaluator(ix, _kparams(m, cfg)).completeness_pieces()
    tot = 0.0
    for piece in range(64):
        lo, hi = piece << (2 * k - 6), (piece + 1) << (2 * k - 6)
        rs, as_ = (read[0] >= lo) & (read[0] < hi), (asm[0] >= lo) & (asm[0] < hi)
        want = po.completeness_piece(p, read[0][rs], read[1][rs], asm[0][as_], asm[1][as_])
        assert (t64[piece], u64[piece]) == want, piece
        tot += want[0]
    assert tot > 0


def test_saturation_tiles_of_the_packed_word(monkeypatch):
    """k = 21, sequence-only compact: a lane's koverCpy sum of a tile (56 bits) and its dominant-bin count (8 bits) share one LDS
    word.  Contig A: every k-mer adds a term of 1 - 1/2046, 16 per lane and tile -- the sum just below 2^56, the count 0.  B: every
    k-mer in the dominant bin -- the count 16.  C: both, alternating by position.  D: assembly counts beyond the 11-bit fields --
    the same words fed by mfx_hist_rest_kernel through the side table; with nbins = 1024 whole waves hit one far-bin key."""
    m = _mfx()
    k, n = 21, 2 * PC["tile"] + 20
    cfg = CONFIGS["peak17.3"]
    A, B, D = (5, PC["field"] - 1), (17, 1), (5, 40000)
    w = kg.build_world(k, None, seed=5, uniform=[(n, A), (n, B), (n, [A, B]), (n, D)])
    ref = kg.reference(w, cfg)
    assert ref.contig_kasm == [2 * PC["tile"]] * 4 and ref.contig_n_under == [2 * PC["tile"], 0, PC["tile"], 2 * PC["tile"]]
    assert ref.over == {0: 3 * PC["tile"]} and len(ref.undr) == 2 and max(ref.undr) > 65536
    _roomy_side_table(monkeypatch, w)
    ix, seqs, _, _ = _build(m, w, "seq", k)
    for nbins in (0, PC["nb_lds"]):
        ev = m.Evaluator(ix, _kparams(m, cfg), nbins=nbins)
        for rep in range(2):
            assert_matches(ev.hist(seqs), ref, "seq", _ntiles(w), "saturation nbins=%d run %d" % (nbins, rep))
    # each contig alone (a sequence-only index is bound to its sequence: one index per contig), so that the words of a launch are of
    # one kind only
    read, asm = kg.tables(w)
    for ci in range(4):
        w1 = kg.World()
        w1.k, w1.contigs, w1.kmers, w1.R, w1.A = k, [w.contigs[ci]], [w.kmers[ci]], w.R, w.A
        r1 = kg.reference(w1, cfg)
        ix1, seqs1 = seq_index(m, k, w1.contigs, read, asm)
        assert ix1.info()["compact"]
        for nbins in (0, PC["nb_lds"]):
            assert_matches(m.Evaluator(ix1, _kparams(m, cfg), nbins=nbins).hist(seqs1), r1, "seq", _ntiles(w1), "saturation contig %d nbins=%d" % (ci, nbins))
