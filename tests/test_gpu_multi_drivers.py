"""The five one-process drivers that run -hist over several slots and put the slots' results together (csrc/mfx_multi.cpp:
mfx_hist_run_multi, mfx_hist_run_streamed_multi, mfx_hist_run_parts, both forms of mfx_hist_run_sharded) on ONE world whose K* histogram
reaches far beyond the dense device image on both sides and in every slot's share: each driver's reduction must carry every slot's
overflow list, its per-contig counters (scattered, for the parts) and its koverCpy through, and a call the driver refuses must leave
the objects fit for the next one.  All slots are contexts on device 0.

Two contigs of 770 tiles: the smallest size at which the streamed shares of two slots (cut at multiples of 1024 tiles) are both
non-empty, so the hot k-mers at the four contig ends fall into different slots in every driver."""
import numpy as np
import pytest

from tests.overflow_world import overflow_world
from tests.test_gpu_parity import assert_hist_equal, build_index, oracle_hist
from tests.test_gpu_parts import build_parts
from tests.test_gpu_sharded import _build_shards

pytestmark = pytest.mark.gpu
TILES = 770
PER = 256             # tiles a shard routes per round: the world's ~1540 tiles over 2 or 3 shards are 4 or 3 rounds


class World:
    def __init__(self, m):
        self.k, self.peak, self.contigs, self.read, self.asm = overflow_world(TILES)
        _, self.g, self.ka, self.km = oracle_hist(self.k, self.peak, self.contigs, self.read, self.asm)
        self.lens = [len(c) for c in self.contigs]
        self.kp = m.KParams(self.peak)
        self.ix = build_index(m, self.k, self.read, self.asm)
        self.seqs = m.Sequences(self.contigs)
        self.resident = m.Evaluator(self.ix, self.kp).hist(self.seqs)

    def check(self, res):
        assert_hist_equal(res, self.g, self.ka, self.km, self.k)


@pytest.fixture(scope="module")
def world():
    import merfin_amd as m
    return World(m)


# Every leg: {label: [first call, second call on the same objects]}, each pair made right after a call on those objects that the
# driver refuses (an argument refusal, before anything is launched).  setenv(name, value) sets an environment variable for the leg.
def leg_multi(m, W, n, setenv):
    evs = [m.Evaluator(W.ix, W.kp) for _ in range(n)]
    with pytest.raises(m.MfxError):                              # an evaluator twice
        m.hist_multi([evs[0]] + evs[:-1], [W.seqs] * n)
    return {"multi": [m.hist_multi(evs, [W.seqs] * n) for _ in range(2)]}


def leg_streamed_multi(m, W, n, setenv):
    evs = [m.Evaluator(W.ix, W.kp) for _ in range(n)]
    sqs = [m.Sequences.create(W.lens) for _ in range(n)]
    with pytest.raises(m.MfxError, match="share an evaluator or a sequence"):
        m.hist_streamed_multi([evs[0]] + evs[:-1], sqs, W.contigs)
    return {"streamed_multi": [m.hist_streamed_multi(evs, sqs, W.contigs) for _ in range(2)]}


def leg_parts(m, W, n, setenv):
    ixs, seqs, ids = build_parts(m, W.k, W.contigs, W.read, n, asm_db=W.asm)
    assert sorted(ids) == [[0], [1]]                             # one contig each
    evs = [m.Evaluator(ix, W.kp) for ix in ixs]
    out = {}
    for label, order in (("parts ids [[0], [1]]", sorted(range(n), key=lambda d: ids[d])), ("parts ids [[1], [0]]", sorted(range(n), key=lambda d: -ids[d][0]))):
        e, s, i = [evs[d] for d in order], [seqs[d] for d in order], [ids[d] for d in order]
        with pytest.raises(m.MfxError, match="two slots|out of range"):      # a contig number in two parts
            m.hist_parts(e, s, [i[0], i[0]], len(W.contigs))
        out[label] = [m.hist_parts(e, s, i, len(W.contigs)) for _ in range(2)]
    return out


def leg_sharded(m, W, n, setenv):
    shards = _build_shards(m, W.k, W.read, W.asm, n)
    evs = [m.Evaluator(s, W.kp) for s in shards]
    routers = [m.Router(s, n, PER) for s in shards]
    per_shard = -(-W.seqs.ntiles // n)
    assert -(-per_shard // PER) >= 3                             # rounds of a run
    out = {}
    for form, ordered in (("sharded fused", "0"), ("sharded ordered", "1")):
        setenv("MFX_SHARDED_ORDERED", ordered)
        with pytest.raises(m.MfxError):                          # the slots must be shard 0..N-1 in order
            m.hist_sharded(evs[::-1], routers[::-1], [W.seqs] * n)
        out[form] = [m.hist_sharded(evs, routers, [W.seqs] * n) for _ in range(2)]
    return out


LEGS = {"multi-2": (leg_multi, 2), "multi-3": (leg_multi, 3), "streamed_multi-2": (leg_streamed_multi, 2), "streamed_multi-3": (leg_streamed_multi, 3),
        "parts-2": (leg_parts, 2), "sharded-2": (leg_sharded, 2), "sharded-3": (leg_sharded, 3)}


def test_the_world_reaches_every_slot(world):
    import merfin_amd as m
    W = world
    assert W.g.c.undrMax > 65536 and W.g.c.overMax > 65536       # far bins on both sides
    for r in range(2):
        lo, hi = m.stream_share(W.seqs.ntiles, r, 2)
        assert hi > lo                                           # both streamed shares hold tiles
    assert W.seqs.ntiles > 256 * 3                               # every slot of three gets 256-tile blocks of the cyclic deal
    W.check(W.resident)


@pytest.mark.parametrize("leg", sorted(LEGS))
def test_driver_equals_the_oracle_far_bins_included(leg, world, monkeypatch):
    import merfin_amd as m
    fn, n = LEGS[leg]
    runs = fn(m, world, n, monkeypatch.setenv)
    for label, (first, second) in runs.items():
        world.check(first)
        world.check(second)
        assert second.koverCpy.hex() == first.koverCpy.hex(), label      # the same objects again: the same bits
    if fn is leg_streamed_multi:
        # the shares are cut where the single launch cuts its first-level sums: koverCpy is the resident run's, bit for bit
        assert runs["streamed_multi"][0].koverCpy.hex() == world.resident.koverCpy.hex()
    if fn is leg_sharded:
        a, b = runs["sharded fused"][0], runs["sharded ordered"][0]
        assert (a.kasm, a.kmissing) == (b.kasm, b.kmissing)
        for f in ("undr", "over", "contig_kasm", "contig_kmissing"):
            np.testing.assert_array_equal(getattr(a, f)(), getattr(b, f)())
