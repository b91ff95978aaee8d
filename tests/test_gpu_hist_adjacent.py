"""-hist with a wave on ADJACENT stretches of a tile, the koverCpy sums kept per slot.

mfx_hist_kernel gives wave v of a block the cells v BT .. v BT + BT - 1 of a batch (a cell: 64 consecutive positions; BT = 2 for the
k = 21 and k = 31 instances, 4 for the generic ones), so a wave holds 128 or 256 contiguous positions and the seams between cells at
64, 128, 256 and 512 positions are seams of another kind than they were: inside a wave (its halo is the next cell's first t-mers),
between two waves, between two batches.  The SLOT of a position -- the (tile, slot) word of its koverCpy term, and the worklist's --
stays (p % 256) // 64, whichever wave holds it; the sums live in four LDS words per block.

  1. oracle parity on contigs whose lengths sit around every such seam, with N, lower case, a repeat (asmK > readK: koverCpy terms)
     and, for even k, own-reverse-complement k-mers AT the seams; every instance of the kernel; launches by ranges and cyclic shares.
     koverCpy within the bound tests/test_gpu_hist_tile_seams.py derives (kover_bar).
  2. the grouping of the terms pinned by BITS: a world whose every (tile, slot) integer exceeds 2^53, so that its conversion to a double
     rounds and the rounding depends on which terms share a word.  The reference is plain Python -- tests/kstar_grid.py's exact integer
     terms, summed per (tile, (p % 256) // 64), converted as float(u) * 2^-52 and added in the order of mfx_sum_chunks_kernel<true> and
     mfx_sum_partials_kernel -- and the device's koverCpy must equal it bit for bit, for the whole launch and for every tile launched
     alone.  The test asserts from its own reference that a grouping by the PHYSICAL wave ((p % 256) // 128 holds cells 2v, 2v + 1 at
     BT = 2) gives other bits on this world.
     Recorded once on a scratch build that wrote the physical wave's number into the slot (an MI355X): see docs/HISTORY.md.
  3. the worklist's slots on the k = 21 and k = 22 worlds of tests/worklist_world.py, segments of 3 entries and the default: every
     listed entry's slot holds its k-mer (World.slot_kmers), the result equals the unlisted run's bit for bit."""
import numpy as np
import pytest

from tests import kstar_grid as kg
from tests import synth
from tests import worklist_world as ww
from tests.test_gpu_hist_tile_seams import ROUTES, _tables, kover_bar
from tests.test_gpu_kstar_grid import _kparams
from tests.test_gpu_parity import assert_hist_equal, build_index, oracle_hist
from tests.test_gpu_second_bucket import assert_same_run
from tests.test_gpu_seqonly import seq_index
from tests.test_gpu_worklist import check_list
from tests.test_gpu_worklist import _index as worklist_index
from tests.test_kstar_grid_cpu import CONFIGS, PC

pytestmark = pytest.mark.gpu

PEAK = 17.3
TILE, BLOCK = PC["tile"], PC["block"]
SLOTS = BLOCK // 64
SEAMS = (64, 128, 256, 512)
MARKS = (63, 64, 127, 128, 255, 256, 511, 512)
LENGTHS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8197)
_RC = bytes.maketrans(b"ACGT", b"TGCA")
_worlds = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


# ---------------------------------------------------------------------------
# 1. oracle parity
# ---------------------------------------------------------------------------
def _contigs(k, seed):
    """contigs of k - 1 + L bases, L k-mers each; three more of L = 8197 carry the marks (one per shift 0, -1, +1).  The first long
    contig: a repeated unit across every seam of both its tiles.  The marked ones: N at the marks of tile 0; in tile 1 (even k) an
    own-reverse-complement k-mer across every seam, then lower case at the marks."""
    r = synth.rng(seed)
    lens = [k - 1 + L for L in LENGTHS] + [k - 1 + 8197] * 3
    c = [synth.random_contig(r, n) for n in lens]
    long0 = len(LENGTHS) - 1
    unit = synth.random_contig(r, k + 27)
    for tile in (0, 1):
        for s in SEAMS:
            at = tile * TILE + s - len(unit) // 2
            c[long0][at:at + len(unit)] = unit                 # its k-mers start on both sides of the seam
    for j, shift in enumerate((0, -1, 1)):
        x = c[long0 + 1 + j]
        for p in MARKS:
            x[p + shift] = ord("N")
        if k % 2 == 0:
            for s in SEAMS:
                h = synth.random_contig(r, k // 2).tobytes()
                at = TILE + s - k // 2 + shift                 # starts before the seam, ends behind it
                x[at:at + k] = np.frombuffer(h + h.translate(_RC)[::-1], dtype=np.uint8)
        for p in MARKS:
            x[TILE + p + shift] |= 0x20
    c[long0][TILE + 60:TILE + 70] |= 0x20                      # lower case on a repeat across a seam
    return synth.as_bytes(c)


def _world(k):
    """one world and its oracle result per k, shared by every test here; unchanged"""
    if k not in _worlds:
        contigs = _contigs(k, 8100 + k)
        read, asm = _tables(k, contigs, 8200 + k)
        _, g, ka, km = oracle_hist(k, PEAK, contigs, read, asm)
        assert len(ka) == len(LENGTHS) + 3 and list(ka[:len(LENGTHS)]) == list(LENGTHS)      # (the unmarked contigs: every position a k-mer)
        assert g.kmissing > 100 and g.koverCpy > 50.0
        _worlds[k] = (contigs, read, asm, g, ka, km)
    return _worlds[k]


def _ntiles(contigs):
    return sum((len(c) + TILE - 1) // TILE for c in contigs)


def _index(m, route, monkeypatch, seqs):
    k, kind, env = ROUTES[route]
    contigs, read, asm, g, ka, km = _world(k)
    for a, b in env.items():
        monkeypatch.setenv(a, b)
    if kind == "seq":
        ix, _ = seq_index(m, k, contigs, read, asm, seqs=seqs)
        assert ix.info()["compact"] and ix.info()["seq_only"]
    else:
        ix = build_index(m, k, read, asm)
    for a in env:
        monkeypatch.delenv(a)
    return ix


def _image(m, ev, launch, ncontigs):
    import torch
    counts = torch.zeros(m.hist_words(ev.nbins, ncontigs), dtype=torch.int64, device="cuda")
    kover = torch.zeros(1, dtype=torch.float64, device="cuda")
    launch(counts, kover, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert len(ev.take_overflow()) == 0
    return counts.cpu().numpy().view(np.uint64), float(kover.item())


@pytest.mark.parametrize("route", list(ROUTES))
def test_adjacent_stretches_give_the_oracles_result(route, monkeypatch):
    m = _mfx()
    k, kind, _ = ROUTES[route]
    contigs, read, asm, g, ka, km = _world(k)
    seqs = m.Sequences(contigs)
    ev = m.Evaluator(_index(m, route, monkeypatch, seqs), m.KParams(PEAK))
    T, nc = seqs.ntiles, len(contigs)
    assert T == _ntiles(contigs) and T > 8
    bar = kover_bar(g, T)
    res = ev.hist(seqs)
    err = abs(res.koverCpy - g.koverCpy)
    print("%s: kasm %d kmissing %d koverCpy %.17g, |gpu - oracle| %.3e (bar %.3e)" % (route, res.kasm, res.kmissing, res.koverCpy, err, bar))
    assert_hist_equal(res, g, ka, km, k)
    assert err <= bar, (route, err, bar)
    again = ev.hist(seqs)
    assert np.float64(again.koverCpy).tobytes() == np.float64(res.koverCpy).tobytes()
    # launches that end inside the sequence, and the cyclic deal of 3 ranks: the parts sum to the whole
    whole, kwhole = _image(m, ev, lambda c, kv, st: ev.hist_launch(seqs, 0, T, c, kv, stream=st), nc)
    assert_hist_equal(ev.result_from_counts(whole, kwhole, nc), g, ka, km, k)
    assert np.float64(kwhole).tobytes() == np.float64(res.koverCpy).tobytes()
    tot, ktot = np.zeros_like(whole), 0.0
    for lo, hi in ((0, 1), (1, 3), (3, T - 1), (T - 1, T)):
        a, kva = _image(m, ev, lambda c, kv, st: ev.hist_launch(seqs, lo, hi, c, kv, stream=st), nc)
        tot += a
        ktot += kva
    np.testing.assert_array_equal(tot, whole)
    print("%s: ranges |sum - whole| %.3e" % (route, abs(ktot - kwhole)))
    assert abs(ktot - kwhole) <= bar
    tot, ktot = np.zeros_like(whole), 0.0
    for rank in range(3):
        a, kva = _image(m, ev, lambda c, kv, st: ev.hist_launch_cyclic(seqs, rank, 3, c, kv, block_tiles=1, stream=st), nc)
        assert a[2 * ev.nbins + 0] > 0                               # every share holds k-mers
        tot += a
        ktot += kva
    np.testing.assert_array_equal(tot, whole)
    print("%s: cyclic |sum - whole| %.3e" % (route, abs(ktot - kwhole)))
    assert abs(ktot - kwhole) <= bar


# ---------------------------------------------------------------------------
# 2. the grouping of the terms, by bits
# ---------------------------------------------------------------------------
def device_sum(words):
    """the fp64 sum of 64-bit integer words (units of 2^-52) as mfx_sum_chunks_kernel<true> and mfx_sum_partials_kernel make it: per chunk
    of 4096 words 256 strided running sums of the converted words, a halving tree over the 256; the same over the chunks' sums; added
    to an output that holds 0"""
    def level(vals):
        s = [0.0] * BLOCK
        for t in range(BLOCK):
            for i in range(t, len(vals), BLOCK):
                s[t] = s[t] + vals[i]
        st = BLOCK // 2
        while st > 0:
            for t in range(st):
                s[t] = s[t] + s[t + st]
            st //= 2
        return s[0]
    chunk = 4096
    firsts = [level([float(u) * 2.0 ** -52 for u in words[b:b + chunk]]) for b in range(0, len(words), chunk)]
    return 0.0 + level(firsts)


def _slot_words(w, cfg, group):
    """the integer of every (tile, group(position in the tile)) of the world's one contig, tile-major"""
    (n, pos, f, rr), = w.kmers
    nt = (n + TILE - 1) // TILE
    words = [0] * (nt * SLOTS)
    for p, a, b in zip(pos, f, rr):
        rv, av = w.pair_of[min(a, b)]
        e = kg.evaluate(rv, av, cfg)
        if e[3] == "u":
            words[(p // TILE) * SLOTS + group(p % TILE)] += kg.kfix(e[6])
    return words


@pytest.mark.parametrize("k", [21, 31])
def test_koverCpy_bits_pin_the_slot_grouping(k):
    m = _mfx()
    cfg = CONFIGS["peak17.3"]
    # read count 17 -> readK 1; most positions have asmK > readK, one in seven sits in the dominant bin; seven pairs against cells of 64
    spec = [(17, 3), (17, 40), (17, 1), (17, 7), (17, PC["field"] - 1), (17, 2), (17, 11)]
    n = 2 * TILE + 700 + k - 1
    w = kg.build_world(k, None, seed=40 + k, uniform=[(n, spec)])
    words = _slot_words(w, cfg, lambda p: (p % BLOCK) // 64)
    by_wave = _slot_words(w, cfg, lambda p: (p % (2 * BLOCK)) // 128)      # BT = 2: wave v holds cells 2v, 2v + 1 of a batch of 512
    nt = len(words) // SLOTS
    assert nt == 3 and min(words) > 2 ** 53 and sum(words) == sum(by_wave)
    want = [device_sum(words[t * SLOTS:(t + 1) * SLOTS]) for t in range(nt)] + [device_sum(words)]
    other = [device_sum(by_wave[t * SLOTS:(t + 1) * SLOTS]) for t in range(nt)] + [device_sum(by_wave)]
    differ = [np.float64(a).tobytes() != np.float64(b).tobytes() for a, b in zip(want, other)]
    print("k = %d: words %r; sums by slot %r, by physical wave %r" % (k, words, want, other))
    assert any(differ), "the world does not tell the two groupings apart"
    read, asm = kg.tables(w)
    ix, seqs = seq_index(m, k, w.contigs, read, asm)
    assert ix.info()["compact"] and seqs.ntiles == nt
    ev = m.Evaluator(ix, _kparams(m, cfg))
    got = []
    import torch
    for lo, hi in [(t, t + 1) for t in range(nt)] + [(0, nt)]:
        counts = torch.zeros(m.hist_words(ev.nbins, 1), dtype=torch.int64, device="cuda")
        kover = torch.zeros(1, dtype=torch.float64, device="cuda")
        ev.hist_launch(seqs, lo, hi, counts, kover, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got.append(float(kover.item()))
    whole = ev.hist(seqs)
    print("k = %d: device %r, hist() %.17g" % (k, got, whole.koverCpy))
    assert whole.kasm == n - k + 1 and whole.kmissing == 0
    for a, b in zip(got + [whole.koverCpy], want + [want[-1]]):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (k, got, whole.koverCpy, want)


# ---------------------------------------------------------------------------
# 3. the worklist's slots
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 22])
def test_listed_entries_sit_in_the_slot_of_their_position(k, monkeypatch):
    m = _mfx()
    w, ix, seqs = worklist_index(m, k, {}, monkeypatch)
    ev = m.Evaluator(ix, m.KParams(ww.PEAK))
    ev.debug_worklist(0)
    unlisted = ev.hist(seqs)
    assert ev.debug_worklist_read()[0] == 0
    tiles = np.arange(w.ntiles)
    for mode, cap in ((1, 0), (2, 3)):
        ev.debug_worklist(mode, cap)
        res = ev.hist(seqs)
        segs, segcap, counts, ent = ev.debug_worklist_read()
        cl = check_list(w, segs, segcap, counts, ent, tiles, "k = %d, segments of %d" % (k, segcap))
        print("k = %d: %d segments of %d: %r" % (k, segs, segcap, cl))
        assert cl["listed"] > 0 and (mode == 1 or (segcap == 3 and int(counts.max()) == 3))
        if mode == 1:
            assert len(np.unique((ent["w"] & np.uint32(0x1fffffff)) % SLOTS)) == SLOTS      # every slot of a tile is listed somewhere
        assert_same_run(res, unlisted, "k = %d, segments of %d against the unlisted run" % (k, segcap))
        assert np.float64(res.koverCpy).tobytes() == np.float64(unlisted.koverCpy).tobytes()
    ev.debug_worklist(1)
