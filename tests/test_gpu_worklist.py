"""The -hist worklist (mfx_hist_kernel's push_wave, mfx_hist_rest_kernel): over a compact, canonical table the main kernel LISTS the rare
endings of its probe -- queries displaced past the two cooperative passes (mode 0 home line, 1 deep), saturated 11-bit fields whose
side-table entry is not in the first two slots of its side line (mode 2) -- in one segment per block, and the rest kernel ends them; a
lane whose entry does not fit its segment, or a launch without a list, scans for itself.  The kernel's comment promises the result "the
main kernel alone would have produced, bit for bit, whatever was listed".  Here, on the worlds of tests/worklist_world.py (saturated read
counts on ~3000 k-mers, saturated palindromes at even k, a read filter that makes listed k-mers missing, a short last tile):

  a) every instance (k = 21 specialised and generic, 19, 20, 22, 26, 31; -prob at k = 21 and 31) under every list setting -- default, off
     by the test hook, MFX_HIST_WORKLIST=0, segments capped at 1, 63, 64, 65, 200 entries (mfx_eval_debug_worklist) -- against the oracle:
     every integer `==`, the far bins through take_overflow (a second evaluation at peak 5, nbins = 1024), a second run equal, koverCpy of
     every setting bit-equal to the default's, the default's within the bound derived in tests/test_gpu_second_bucket.py's docstring;
  b) the list itself read back (mfx_eval_debug_worklist_read), default and segcap = 65: every entry's k-mer is the canonical k-mer of a
     position of its own (tile, wave), no (k-mer, slot) more often than the wave has it, `dbl` iff the k-mer is its own reverse complement,
     mode 2 only for saturated k-mers, segment b only tile b's slots, counts <= segcap, a full segment under the cap where the default
     listed more, fewer entries than the default and more than none;
  c) the classes occur: modes 0 / 1, mode 2, `dbl` at even k, a listed k-mer that evaluates to missing;
  d) the launch forms over the same index (k = 21, 22, 31; default, off, segcap = 65): tile ranges, block-cyclic shares (the rest kernel's
     part_n > 1 arithmetic -- its list is read back too), the streamed run whole and by ranges, three slots: integers `==` the whole
     launch, koverCpy bit-equal to the same form under the default list.

The issue behind this file names k = 22 and k = 26 as "direct and quotient form"; the compact layout holds the k-mer itself only for
k <= 21 (MFX_MAX_K_DIRECT), so both are quotient tables and k = 20 is here as the even k of the direct form.  A world of this size is
ONE chunk of the streamed run (its first chunk is 2048 tiles) and one share of mfx_hist_run_streamed_multi (shares are multiples of
1024 tiles): the streamed run is cut by hist_streamed_range, whose parts the caller sums (rel 1e-12, as the caller-summed ranges)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import worklist_world as ww
from tests.test_gpu_second_bucket import _prob, _trim, assert_equals_oracle, assert_same_run
from tests.test_gpu_seqonly import seq_index

pytestmark = pytest.mark.gpu

# instance -> (k, environment)
INSTANCES = {"k21": (21, {}), "k21_generic": (21, {"MFX_HIST_GENERIC": "1"}), "k19": (19, {}), "k20": (20, {}), "k22": (22, {}), "k26": (26, {}), "k31": (31, {})}
CASES = [(name, False) for name in INSTANCES] + [(name, True) for name, (k, _) in INSTANCES.items() if k in (21, 31)]
# setting -> (hook mode, segcap, MFX_HIST_WORKLIST)
SETTINGS = {"default": (1, 0, None), "off": (0, 0, None), "env0": (1, 0, "0"), "cap1": (2, 1, None), "cap63": (2, 63, None), "cap64": (2, 64, None),
            "cap65": (2, 65, None), "cap200": (2, 200, None)}
NB_FAR = 1024
_refs = {}


def _mfx():
    import merfin_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def reference(k, peak, use_prob):
    """the oracle's run under the read filter, once per (k, peak, -prob); unchanged"""
    if (k, peak, use_prob) not in _refs:
        w = ww.world(k)
        probK, probP = _prob(use_prob)
        g, ka, km, _ = po.hist_run(po.Params(k, peak, probK, probP), po.Lookup(k, w.read[0], w.read[1], 0, ww.READ_MAX), po.Lookup(k, *w.asm), w.contigs,
                                   threads=4, mode=0)
        _refs[(k, peak, use_prob)] = (g, ka, km)
    return _refs[(k, peak, use_prob)]


def far_records(g, nbins):
    """{key: occurrences} of the oracle's bins >= nbins as Evaluator.take_overflow reports them (bit 63: `over`)"""
    u, o = np.asarray(g.undr()), np.asarray(g.over())
    want = {i: int(u[i]) for i in range(nbins, len(u)) if u[i]}
    want.update({(1 << 63) | i: int(o[i]) for i in range(nbins, len(o)) if o[i]})
    return want


def assert_far_equals_oracle(res, ref, ntiles, what):
    """The second evaluation (FAR_PEAK) against the oracle: every integer `==`, koverCpy within the bound of
    tests/test_gpu_second_bucket.py's docstring.  assert_equals_oracle itself also asks for more than 100 under-represented k-mers, which
    holds at PEAK; at peak 5 nearly every read count exceeds its assembly count (n_under is about ten) and what this evaluation is
    here for are the `over` bins beyond nbins, asserted where it is called."""
    g, ka, km = ref
    assert (res.kasm, res.kmissing) == (g.kasm, g.kmissing), what
    np.testing.assert_array_equal(_trim(res.undr()), _trim(g.undr()), err_msg=what)
    np.testing.assert_array_equal(_trim(res.over()), _trim(g.over()), err_msg=what)
    np.testing.assert_array_equal(res.contig_kasm(), ka, err_msg=what)
    np.testing.assert_array_equal(res.contig_kmissing(), km, err_msg=what)
    n_under, S = int(np.asarray(g.undr()).sum(dtype=np.uint64)), float(g.koverCpy)
    bound = (n_under + (ww.WAVES * ntiles + 64) * S) * 2.0 ** -53 + n_under * S * 2.0 ** -53
    err = abs(res.koverCpy - S)
    print("%s: kasm %d kmissing %d n_under %d koverCpy %.9f |got - oracle| %.3e (bound %.3e)" % (what, res.kasm, res.kmissing, n_under, S, err, bound))
    assert g.kmissing > 0 and err <= bound, (what, err, bound)


def _index(m, k, env, monkeypatch):
    """host-built tables: the oracle's assembly counts, the read database under -max through the index's filter"""
    monkeypatch.setenv("MFX_LOAD_FACTOR", "0.5")
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    w = ww.world(k)
    ix, seqs = seq_index(m, k, w.contigs, w.read, asm=w.asm, lo=0, hi=ww.READ_MAX)
    info = ix.info()
    assert info["seq_only"] and info["compact"] and info["distinct"] == len(w.asm[0]) and seqs.ntiles == w.ntiles
    return w, ix, seqs


class setting:
    """a list setting on some evaluators for the length of a `with`"""

    def __init__(self, monkeypatch, name, *evs):
        self.mp, self.name, self.evs = monkeypatch, name, evs

    def __enter__(self):
        mode, segcap, env = SETTINGS[self.name]
        for ev in self.evs:
            ev.debug_worklist(mode, segcap)
        if env is not None:
            self.mp.setenv("MFX_HIST_WORKLIST", env)

    def __exit__(self, *exc):
        self.mp.delenv("MFX_HIST_WORKLIST", raising=False)
        for ev in self.evs:
            ev.debug_worklist(1)


def _launch_by_hand(m, torch, ev, seqs):
    counts = torch.zeros(m.hist_words(ev.nbins, seqs.ncontigs), dtype=torch.int64, device="cuda")
    kover = torch.zeros(1, dtype=torch.float64, device="cuda")
    ev.hist_launch(seqs, 0, seqs.ntiles, counts, kover, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return counts.cpu().numpy().view(np.uint64), float(kover.item())


# ---- a) the invariant ----
@pytest.mark.parametrize("name,use_prob", CASES, ids=["%s-%s" % (n, "prob" if p else "noprob") for n, p in CASES])
def test_every_list_setting_gives_the_oracles_result_bit_for_bit(name, use_prob, monkeypatch):
    torch = pytest.importorskip("torch")
    m = _mfx()
    k, env = INSTANCES[name]
    w, ix, seqs = _index(m, k, env, monkeypatch)
    ref, ref_far = reference(k, ww.PEAK, use_prob), reference(k, ww.FAR_PEAK, use_prob)
    far = far_records(ref_far[0], NB_FAR)
    assert sum(far.values()) >= 500
    ev = m.Evaluator(ix, m.KParams(ww.PEAK, *_prob(use_prob)))
    ev_far = m.Evaluator(ix, m.KParams(ww.FAR_PEAK, *_prob(use_prob)), nbins=NB_FAR)
    base = base_far = None
    for s in SETTINGS:
        what = "%s prob=%d %s" % (name, use_prob, s)
        with setting(monkeypatch, s, ev, ev_far):
            first = ev.hist(seqs)
            segs, segcap, counts, _ = ev.debug_worklist_read()
            again = ev.hist(seqs)
            # the far bins: folded into the result by hist(), and taken by hand behind a plain launch
            res_far = ev_far.hist(seqs)
            assert len(ev_far.take_overflow()) == 0
            h, kv = _launch_by_hand(m, torch, ev_far, seqs)
            rec = ev_far.take_overflow()
        print("%s: %d segments of %d, %d listed" % (what, segs, segcap, int(counts.sum())))
        mode, cap, envv = SETTINGS[s]
        assert (segs == 0) == (mode == 0 or envv == "0"), what                  # the setting took effect
        assert mode != 2 or (segcap == cap and int(counts.max()) <= cap), what
        assert_equals_oracle(first, ref, k, seqs.ntiles, what)
        assert_same_run(again, first, what + ", second run")
        assert_far_equals_oracle(res_far, ref_far, seqs.ntiles, what + " far")
        assert {int(a): int(b) for a, b in rec} == far and len(rec) == len(far), what
        assert int(h[2 * ev_far.nbins + 2]) == sum(far.values()), what
        by_hand = ev_far.result_from_counts(h, kv, seqs.ncontigs).add_overflow(rec)
        _ints_equal(by_hand, res_far, what + " far, by hand")
        assert by_hand.koverCpy == res_far.koverCpy, what
        if s == "default":
            base, base_far = first, res_far
        else:
            assert np.float64(first.koverCpy).tobytes() == np.float64(base.koverCpy).tobytes(), (what, first.koverCpy, base.koverCpy)
            assert np.float64(res_far.koverCpy).tobytes() == np.float64(base_far.koverCpy).tobytes(), (what, res_far.koverCpy, base_far.koverCpy)
            assert_same_run(first, base, what + " against the default")


# ---- b), c) the list read back ----
def _revcomp(km, k):
    r = np.zeros(len(km), dtype=np.uint64)
    x = km.copy()
    for _ in range(k):
        r = (r << np.uint64(2)) | ((x & np.uint64(3)) ^ np.uint64(2))
        x >>= np.uint64(2)
    return r


def check_list(w, segs, segcap, counts, ent, tile_of_li, what, seg_is_tile=True):
    """every property of b) that one list has by itself; returns its class counts.  tile_of_li: the launch's tile numbering -> the
    sequence's tile"""
    assert len(counts) == segs and int(counts.sum()) == len(ent) and (counts <= segcap).all(), what
    slot = (ent["w"] & np.uint32(0x1fffffff)).astype(np.int64)
    mode = (ent["w"] >> np.uint32(29)) & np.uint32(3)
    dbl = (ent["w"] >> np.uint32(31)).astype(bool)
    li, wave = slot // ww.WAVES, slot % ww.WAVES
    assert mode.max(initial=0) <= 2, what
    if seg_is_tile:                                                  # grid >= tiles of the launch: block b has tile b and nothing else
        assert segs == len(tile_of_li), (what, segs)
        np.testing.assert_array_equal(li, np.repeat(np.arange(segs), counts.astype(np.int64)), err_msg=what)
    assert li.max(initial=0) < len(tile_of_li), what
    tile = np.asarray(tile_of_li, dtype=np.int64)[li]
    # its k-mer is a k-mer of its own (tile, wave), and is not listed there more often than the wave has it
    have = w.slot_kmers()
    key = tile * ww.WAVES + wave
    o = np.lexsort((ent["kmer"], key))
    ks, kk = key[o], ent["kmer"][o]
    start = np.concatenate([[0], np.nonzero((np.diff(ks) != 0) | (np.diff(kk) != 0))[0] + 1]) if len(ks) else np.zeros(0, dtype=np.int64)
    mult = np.diff(np.concatenate([start, [len(ks)]]))
    for s, n in zip(start, mult):
        t, v, x = int(ks[s]) // ww.WAVES, int(ks[s]) % ww.WAVES, kk[s]
        pool = have.get((t, v), np.zeros(0, dtype=np.uint64))
        avail = int(np.searchsorted(pool, x, side="right") - np.searchsorted(pool, x, side="left"))
        assert 0 < n <= avail, "%s: k-mer %#x listed %d times in tile %d wave %d, which has it %d times" % (what, int(x), int(n), t, v, avail)
    pal = _revcomp(ent["kmer"], w.k) == ent["kmer"]
    np.testing.assert_array_equal(dbl, pal, err_msg=what)
    assert w.k % 2 == 0 or not dbl.any(), what
    assert np.isin(ent["kmer"][mode == 2], w.sat).all(), what
    at = np.searchsorted(w.asm[0], ent["kmer"])
    rd = w.asm_read[at]
    missing = (rd == 0) | (rd > ww.READ_MAX)
    return {"listed": len(ent), "mode0": int((mode == 0).sum()), "mode1": int((mode == 1).sum()), "mode2": int((mode == 2).sum()), "dbl": int(dbl.sum()),
            "missing": int(missing.sum()), "missing_mode2": int((missing & (mode == 2)).sum())}


@pytest.mark.parametrize("name", list(INSTANCES))
def test_the_list_read_back(name, monkeypatch):
    """Counts observed on an MI355X: docs/HISTORY.md.  The recipe of the issue produced every class at every k as it stands (N_SAT = 3000
    k-mers, MFX_SIDE_DIV at its default)."""
    m = _mfx()
    k, env = INSTANCES[name]
    w, ix, seqs = _index(m, k, env, monkeypatch)
    ev = m.Evaluator(ix, m.KParams(ww.PEAK))
    tiles = np.arange(w.ntiles)
    got = {}
    for s in ("default", "cap65"):
        with setting(monkeypatch, s, ev):
            ev.hist(seqs)
            segs, segcap, counts, ent = ev.debug_worklist_read()
        got[s] = (counts, check_list(w, segs, segcap, counts, ent, tiles, "%s %s" % (name, s)))
        print("%s %s: %d segments of %d: %r" % (name, s, segs, segcap, got[s][1]))
    (cd, d), (cc, c) = got["default"], got["cap65"]
    assert (cc <= 65).all() and ((cc == 65) & (cd > 65)).any(), (name, cc.max(), cd.max())       # a full segment whose tile wanted more
    assert 0 < c["listed"] < d["listed"], (c, d)
    # c) the classes: in the default list, and those that a cap cannot lose in the capped one as well
    assert d["mode0"] + d["mode1"] >= 1 and d["mode2"] >= 1 and d["missing"] >= 1, d
    assert c["mode2"] >= 1 and c["missing"] >= 1, c
    if k % 2 == 0:
        assert d["dbl"] >= 1, d
    # a second evaluator with no setting made at all reads back as the default does
    ev2 = m.Evaluator(ix, m.KParams(ww.PEAK))
    ev2.hist(seqs)
    segs2, segcap2, counts2, _ = ev2.debug_worklist_read()
    assert segs2 == w.ntiles and (counts2 == cd).all()                # (block b of a launch of <= grid tiles has tile b alone)
    assert ev2.debug_worklist_read(1)[0] == 0                          # the second launch slot was not used
    with pytest.raises(m.MfxError):
        ev.debug_worklist(2, 0)
    with pytest.raises(m.MfxError):
        ev.debug_worklist(3, 5)


# ---- d) the launch forms ----
def _ints_equal(res, whole, what):
    assert (res.kasm, res.kmissing) == (whole.kasm, whole.kmissing), what
    np.testing.assert_array_equal(_trim(res.undr()), _trim(whole.undr()), err_msg=what)
    np.testing.assert_array_equal(_trim(res.over()), _trim(whole.over()), err_msg=what)
    np.testing.assert_array_equal(res.contig_kasm(), whole.contig_kasm(), err_msg=what)
    np.testing.assert_array_equal(res.contig_kmissing(), whole.contig_kmissing(), err_msg=what)


def _forms(m, torch, w, ev, evs, seqs, s, name):
    """every launch form over the same index under the setting in force: {form: result}; the lists of the cyclic launches are checked on
    the way"""
    T = seqs.ntiles
    words = m.hist_words(ev.nbins, seqs.ncontigs)
    stream = torch.cuda.current_stream().cuda_stream
    fresh = lambda: (torch.zeros(words, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"))
    result = lambda c, kv: ev.result_from_counts(c.cpu().numpy().view(np.uint64), float(kv.item()), seqs.ncontigs)
    out = {}
    for n in (2, 3, 8):                                              # caller-summed tile ranges
        c, kv = fresh()
        for r in range(n):
            ev.hist_launch(seqs, T * r // n, T * (r + 1) // n, c, kv, stream=stream)
        torch.cuda.synchronize()
        out["%d ranges" % n] = result(c, kv)
    # block-cyclic shares: the rest kernel maps a listed entry's slot back to its tile through part_rank / part_n / part_shift
    for nranks, blk in ((2, 1), (3, 4), (5, 2)):
        c, kv = fresh()
        listed = 0
        for r in range(nranks):
            ev.hist_launch_cyclic(seqs, r, nranks, c, kv, block_tiles=blk, stream=stream)
            segs, segcap, counts, ent = ev.debug_worklist_read()
            mine = [t for t in range(T) if (t // blk) % nranks == r]          # the share's tiles in the order the launch numbers them
            if s in ("off", "env0"):
                assert segs == 0
            else:
                cl = check_list(w, segs, segcap, counts, ent, mine, "%s %s: rank %d of %d, blocks of %d" % (name, s, r, nranks, blk))
                listed += cl["listed"]
                assert cl["missing"] >= 1, cl                        # (every share has listed k-mers above -max)
        torch.cuda.synchronize()
        assert s in ("off", "env0") or listed > 0
        out["cyclic %d x %d" % (nranks, blk)] = result(c, kv)
    lens = [len(c) for c in w.contigs]
    out["streamed"] = ev.hist_streamed(m.Sequences.create(lens), w.contigs)
    c, kv = fresh()
    sq = m.Sequences.create(lens)
    for r in range(3):
        ev.hist_streamed_range(sq, w.contigs, T * r // 3, T * (r + 1) // 3, c, kv)
    torch.cuda.synchronize()
    out["streamed in 3 ranges"] = result(c, kv)
    out["3 slots"] = m.hist_multi(evs, [seqs] * 3)
    return out


@pytest.mark.parametrize("s", ["default", "off", "cap65"])
@pytest.mark.parametrize("name", ["k21", "k22", "k31"])
def test_launch_forms_equal_the_whole_launch(name, s, monkeypatch):
    """Integers `==` the whole launch under every setting.  koverCpy: the streamed run sums the whole launch's (tile, wave) words in the
    whole launch's order -- bit-equal to it; the ranges and shares are summed by the caller and the three slots' shares by
    mfx_hist_run_multi in slot order, other roundings than the whole launch's -- rel 1e-12 against it, and bit-equal to the SAME form
    under the default list, which is the worklist's promise for them."""
    torch = pytest.importorskip("torch")
    m = _mfx()
    k, env = INSTANCES[name]
    w, ix, seqs = _index(m, k, env, monkeypatch)
    ev = m.Evaluator(ix, m.KParams(ww.PEAK))
    evs = [m.Evaluator(ix, m.KParams(ww.PEAK)) for _ in range(3)]
    whole = ev.hist(seqs)                                            # (default list)
    assert_equals_oracle(whole, reference(k, ww.PEAK, False), k, seqs.ntiles, name)
    base = _forms(m, torch, w, ev, evs, seqs, "default", name)
    with setting(monkeypatch, s, ev, *evs):
        got = _forms(m, torch, w, ev, evs, seqs, s, name)
    bits = lambda x: np.float64(x).tobytes()
    for form, res in got.items():
        what = "%s %s: %s" % (name, s, form)
        _ints_equal(res, whole, what)
        if form == "streamed":
            assert bits(res.koverCpy) == bits(whole.koverCpy), (what, res.koverCpy, whole.koverCpy)
        else:
            assert res.koverCpy == pytest.approx(whole.koverCpy, rel=1e-12), what
        assert bits(res.koverCpy) == bits(base[form].koverCpy), (what, res.koverCpy, base[form].koverCpy)
