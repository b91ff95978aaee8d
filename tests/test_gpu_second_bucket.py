"""The second mini-bucket step of the per-lane probe (mfx_lane_front in mfx_kernels.hip): a query that meets neither its key nor
an empty slot in its first mini-bucket reads the next one of its order, (b0 + 1) & 7 of the same line, before it goes to the
cooperative passes.  The k = 31 instance (deferred tail) takes the step; the front of the probe, its one decode and the guard of the
cooperative tail are shared by every caller.  Worlds of < 300 kb in three contigs at MFX_LOAD_FACTOR=0.5 -- the compact layout's upper end, where a fifth of
the k-mers are displaced -- with a diverged satellite array (many distinct k-mers that share their minimizer's window: home lines
full of other k-mers, queries beyond the second mini-bucket, the second cooperative pass), an exact tandem array (read counts beyond
the slot's 11-bit fields: the side table), N runs, lower case and short last tiles.  Every -hist route that calls the probe, with
and without -prob, against oracle/pyoracle.py on HOST-built tables (the read database as generated, the assembly's k-mers counted by
the oracle): every integer `==`; koverCpy within the derived bound below; a second run equal to the first.

koverCpy bound (tests/kstar_grid.py, docs/HISTORY.md): the device adds each term rounded to 2^-52 units into one integer word per
(tile, wave), converts the W = (MFX_BLOCK / 64) * ntiles words and sums them in a fixed order:
    |got - S| <= (n_under + (W + 64) * S) * 2^-53
for the exact sum S of the n_under terms; the oracle is a fp64 sum of the same non-negative terms, |oracle - S| <= n_under * 2^-53 * S
in any order.  Hence |got - oracle| <= (n_under + (W + 64) * S) * 2^-53 + n_under * S * 2^-53 with S taken as the oracle's value."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import synth
from tests import track_ref as tr
from tests.test_gpu_parity import build_index
from tests.test_gpu_seqonly import seq_index
from tests.test_kstar_grid_cpu import PC

pytestmark = pytest.mark.gpu

PEAK = 17.3
SIZES = (150001, 98000, 20500)                   # 268 501 bases; none a multiple of the tile: every contig ends in a short tile
# route -> (k, environment)
ROUTES = {"k21": (21, {}), "k21_w5": (21, {"MFX_MZ_W": "5"}), "k21_generic": (21, {"MFX_HIST_GENERIC": "1"}),
          "k19": (19, {}), "k22": (22, {}), "k31": (31, {})}
_worlds, _refs = {}, {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def _revcomp(b):
    return bytes(b.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1])


def world(k):
    """one world per k, shared by the tests that use it; unchanged"""
    if k not in _worlds:
        r = synth.rng(9100 + k)
        truth = synth.make_truth(r, SIZES, tandem=(37, 200))        # an exact tandem array per contig: read counts of ~3500
        # contig 1: a satellite array, 120 copies of a 171-base unit that diverged by 4 % -- a window of the unit is met with many
        # different flanks, i.e. many distinct k-mers that share their minimizer's window and so their home line
        arr = np.tile(synth.random_contig(r, 171), 120)
        mut = r.random(len(arr)) < 0.04
        arr[mut] = synth.BASES[r.integers(0, 4, size=int(mut.sum()))]
        truth[1][30000:30000 + len(arr)] = arr
        pal_at = []
        if k % 2 == 0:                                               # even k: k-mers that are their own reverse complement
            for i in range(12):
                h = synth.random_contig(r, k // 2).tobytes()
                at = 60000 + 500 * i
                truth[0][at:at + k] = np.frombuffer(h + _revcomp(h), dtype=np.uint8)
                pal_at.append(at)
        asm = synth.decorate(r, synth.mutate(r, truth))
        tb, contigs = synth.as_bytes(truth), synth.as_bytes(asm)
        read = synth.read_counts(r, k, tb, PEAK, err_kmers=2000)
        npal = sum(1 for at in pal_at if contigs[0][at:at + k].upper() == _revcomp(contigs[0][at:at + k].upper()))
        assert k % 2 or npal >= 4
        assert sum(len(c) for c in contigs) <= 300000 and any(b"N" * 50 in c for c in contigs)
        assert all(len(c) % PC["tile"] for c in contigs)
        _worlds[k] = (contigs, read, po.count_kmers(k, contigs))
    return _worlds[k]


def _prob(use_prob):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return po.load_kmetric(os.path.join(root, "tests", "golden", "example_lookup_table.txt")) if use_prob else (None, None)


def reference(k, use_prob):
    if (k, use_prob) not in _refs:
        contigs, read, asm = world(k)
        probK, probP = _prob(use_prob)
        g, ka, km, _ = po.hist_run(po.Params(k, PEAK, probK, probP), po.Lookup(k, *read), po.Lookup(k, *asm), contigs, threads=4, mode=0)
        _refs[(k, use_prob)] = (g, ka, km)
    return _refs[(k, use_prob)]


def _index(m, k, env, monkeypatch):
    monkeypatch.setenv("MFX_LOAD_FACTOR", "0.5")
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    contigs, read, _ = world(k)
    ix, seqs = seq_index(m, k, contigs, read)                       # the assembly side counted from the sequence, as bench.py builds it
    info = ix.info()
    assert info["seq_only"] and info["compact"]
    lf = info["distinct"] / (info["bytes"] / 8.0)
    print("k = %d %r: %d distinct k-mers, load factor %.3f" % (k, env, info["distinct"], lf))
    # a quotient table (k > 21) has at least 2^(2 (k - 3) - 31) lines of 16 slots, whatever the load factor asked for (quot_min_lines in
    # mfx_index.cpp: 128 lines at k = 22, 4 GB at k = 31): at k = 31 a world of this size cannot fill it, and the displaced queries of that
    # route are those of the satellite array, whose k-mers share their home lines at any table size
    floor_slots = 16 << (2 * (k - 3) - 31) if k > 21 else 0
    if floor_slots < info["distinct"] / 0.5:
        assert 0.4 < lf < 0.55, lf
    return ix, seqs


def _trim(a):
    return np.trim_zeros(np.asarray(a), "b")


def assert_equals_oracle(res, ref, k, ntiles, what):
    g, ka, km = ref
    assert (res.kasm, res.kmissing) == (g.kasm, g.kmissing), what
    np.testing.assert_array_equal(_trim(res.undr()), _trim(g.undr()), err_msg=what)
    np.testing.assert_array_equal(_trim(res.over()), _trim(g.over()), err_msg=what)
    np.testing.assert_array_equal(res.contig_kasm(), ka, err_msg=what)
    np.testing.assert_array_equal(res.contig_kmissing(), km, err_msg=what)
    n_under, S = int(np.asarray(g.undr()).sum(dtype=np.uint64)), float(g.koverCpy)
    W = (PC["block"] // 64) * ntiles
    bound = (n_under + (W + 64) * S) * 2.0 ** -53 + n_under * S * 2.0 ** -53
    err = abs(res.koverCpy - S)
    print("%s: kasm %d kmissing %d n_under %d koverCpy %.9f |got - oracle| %.3e (bound %.3e)" % (what, res.kasm, res.kmissing, n_under, S, err, bound))
    assert n_under > 100 and S > 0 and g.kmissing > 0, what
    assert err <= bound, (what, err, bound)


def assert_same_run(a, b, what):
    assert (a.kasm, a.kmissing) == (b.kasm, b.kmissing), what
    assert a.koverCpy == b.koverCpy, what
    np.testing.assert_array_equal(np.asarray(a.undr()), np.asarray(b.undr()), err_msg=what)
    np.testing.assert_array_equal(np.asarray(a.over()), np.asarray(b.over()), err_msg=what)
    np.testing.assert_array_equal(a.contig_kasm(), b.contig_kasm(), err_msg=what)
    np.testing.assert_array_equal(a.contig_kmissing(), b.contig_kmissing(), err_msg=what)


@pytest.mark.parametrize("use_prob", [False, True], ids=["noprob", "prob"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_route_equals_the_oracle_at_load_factor_half(route, use_prob, monkeypatch):
    m = _mfx()
    k, env = ROUTES[route]
    ref = reference(k, use_prob)
    ix, seqs = _index(m, k, env, monkeypatch)
    ev = m.Evaluator(ix, m.KParams(PEAK, *_prob(use_prob)))
    first = ev.hist(seqs)
    assert_equals_oracle(first, ref, k, seqs.ntiles, "%s prob=%d" % (route, use_prob))
    assert_same_run(ev.hist(seqs), first, "%s prob=%d, second run" % (route, use_prob))


@pytest.mark.parametrize("use_prob", [False, True], ids=["noprob", "prob"])
@pytest.mark.parametrize("k", [21, 31])
def test_debug_instance_counts_the_second_bucket(k, use_prob, monkeypatch):
    """The two specialised instances have a debug twin that counts the probe's endings.  k = 31 (deferred tail) takes the step: its
    counter shows it at work, and the passes behind it are still reached.  k = 21, the instance the benchmark runs, is built without
    it (slower there: profiles/r07_second_bucket.txt) -- its displaced queries all go to the passes.  Either way the measured
    instance gives the same result bit for bit."""
    m = _mfx()
    ref = reference(k, use_prob)
    ix, seqs = _index(m, k, {}, monkeypatch)
    ev = m.Evaluator(ix, m.KParams(PEAK, *_prob(use_prob)))
    fast = ev.hist(seqs)
    ev.debug(True)
    dbg = ev.hist(seqs)
    c = ev.debug_counters()
    ev.debug(False)
    print("k = %d probe endings: %r" % (k, c))
    assert_equals_oracle(dbg, ref, k, seqs.ntiles, "debug instance k=%d prob=%d" % (k, use_prob))
    assert_same_run(fast, dbg, "measured against debug instance")
    if k == 31:
        assert c["second_bucket"] > 0, c
    assert c["first_pass"] >= c["second_bucket"], c
    assert c["first_pass"] - c["second_bucket"] > 0, c          # in neither of the first two mini-buckets: the first cooperative pass
    assert c["second_pass"] > 0, c                              # the satellite's home lines are full of other k-mers
    assert c["side_table"] > 0, c                               # the tandem array's read counts are beyond the 11-bit field
    assert c["first_pass"] < fast.kasm, c


@pytest.mark.parametrize("k", [21, 31])
def test_dump_and_track_on_the_same_world(k, monkeypatch):
    """-dump and -track call the same probe: raw values against the full table's (its own cooperative probe) and the oracle's totals,
    K* against the oracle's per-position values; -track's records `==` the reduced oracle values"""
    m = _mfx()
    contigs, read, asm = world(k)
    ix, seqs = _index(m, k, {}, monkeypatch)
    kp = m.KParams(PEAK)
    ev = m.Evaluator(ix, kp)
    full = m.Evaluator(build_index(m, k, read, asm), kp)
    p = po.Params(k, PEAK, None, None)
    R, A = po.Lookup(k, *read), po.Lookup(k, *asm)
    pp = []
    for ci, c in enumerate(contigs):
        rk, ak, km, kasm, kmiss = po.process_dump(p, R, A, c)
        rv, av, gkasm, gkmiss = ev.dump_values(seqs, ci, 0, len(c))
        assert (gkasm, gkmiss) == (kasm, kmiss), ci
        frv, fav, _, _ = full.dump_values(seqs, ci, 0, len(c))
        np.testing.assert_array_equal(rv, frv)
        np.testing.assert_array_equal(av, fav)
        for i in range(0, len(c), 997):
            a, b, _ = m.getK(kp, int(rv[i]), int(av[i]))
            assert (a, b, m.getKmetric(a, b)) == (rk[i], ak[i], km[i]), (ci, i)
        pp.append(tr.per_position_c(po, p, R, A, c))
    W = 1000
    want = tr.reduce_windows(pp, W)
    rec, kasm, kmissing = ev.track(seqs, W)
    got = tr.device_records(rec)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    h = ev.hist(seqs)
    assert (kasm, kmissing) == (h.kasm, h.kmissing)
