"""mfx_var_traverse_kernel and mfx_var_score_kernel against the oracle, path by path (Evaluator.debug_score_paths_trv /
debug_score_paths: the production functions mfx_score_paths_trv / mfx_score_paths with everything they leave on the device copied
back).  The variant modes' own tests see these kernels only after bestFilter / bestVariant / ... reduced numM to a minimum and totdk
to a truncated tie-break; here every cluster of tests/var_clusters.py (the hand-written edges + seeded ones; the same that
tests/test_var_clusters_cpu.py runs through the scalar traverse on the host) comes back whole: status, number of paths, the batch
text byte for byte ('\\n' wherever no path was written: no cluster writes outside its room), the path table, the genotype / offset /
length rows, numM, and totdk as BIT PATTERNS -- the build has -ffp-contract=off, the operations are the reference's in the
reference's order and mfx_getK_core is shared, so equality is what the kernel's comment claims; there is no tolerance.
k = 21, 22 (even: palindromes), 31 against the C oracle's lookups; 33 and 64 through its callback form over arbitrary-precision
k-mers (oracle/plain.py), as tests/test_gpu_wide.py does.  With and without a -prob table, need_dk 0 and 1."""
import functools

import numpy as np
import pytest

from tests import var_clusters as vc

pytestmark = pytest.mark.gpu

CASES = [(k, p) for k in (21, 22, 31, 33, 64) for p in (False, True)]


@functools.lru_cache(maxsize=None)
def setup(k, use_prob):
    import merfin_amd as m
    w = vc.world(k, use_prob, 1200 if k <= 31 else 150)
    ix = vc.build_index(m, w)
    ev = m.Evaluator(ix, m.KParams(vc.PEAK, w.probK or None, w.probP or None))
    return w, ix, ev


def binding():
    from merfin_amd import binding as b
    return b


@pytest.mark.parametrize("k,use_prob", CASES)
def test_device_enumerated_clusters_equal_oracle(k, use_prob):
    """the whole list as ONE batch, host part empty: a few thousand path slots, text over many 4096-byte tiles, RANGE and ROOM
    clusters between exact ones"""
    w, ix, ev = setup(k, use_prob)
    b = vc.pack(binding(), w.clusters, w.scored, seed=k)
    assert b.tables.path_cap > 3000 and b.tables.text_end > 5 * 4096 and sorted(set(b.status.tolist())) == [vc.OK, vc.RANGE, vc.ROOM]
    assert (b.np[b.status == vc.OK] < [int(c["path_cap"]) for c in b.tables.cl[b.status == vc.OK]]).any()      # slots the kernel has to close
    o = ev.debug_score_paths_trv(b.host, b.tables, need_dk=True)
    vc.check_traverse(b, o, "k = %d" % k)
    vc.check_scores(b, o["numM"], o["totdk"], "k = %d, prob %s" % (k, use_prob))
    assert len(set(o["totdk"][b.score_care].tolist())) > 50
    o = ev.debug_score_paths_trv(b.host, b.tables, need_dk=False)                # -filter: numM alone
    vc.check_traverse(b, o, "k = %d, need_dk 0" % k)
    vc.check_scores(b, o["numM"], o["totdk"], "k = %d, need_dk 0" % k, need_dk=False)


@pytest.mark.parametrize("k,use_prob", CASES)
def test_behind_a_host_part_and_host_enumerated_form(k, use_prob):
    """the same clusters with a host part in front (table_base, row_base and the text's start are non-zero), and every path in the
    host-enumerated form (mfx_score_paths): equal results"""
    w, ix, ev = setup(k, use_prob)
    ok = [i for i, x in enumerate(w.scored) if vc.status_of(w.clusters[i], x) == vc.OK]
    front = ok[::3]
    rest = [i for i in range(len(w.clusters)) if i not in set(front)]
    pick = lambda idx: ([w.clusters[i] for i in idx], [w.scored[i] for i in idx])
    b = vc.pack(binding(), *pick(rest), *pick(front), seed=k + 100)
    assert b.hp > 100 and b.hv > 100 and len(b.host.text) > 4096
    o = ev.debug_score_paths_trv(b.host, b.tables, need_dk=True)
    vc.check_traverse(b, o, "k = %d, behind a host part" % k)
    vc.check_scores(b, o["numM"], o["totdk"], "k = %d, behind a host part" % k)
    # host-enumerated: all of them
    h = vc.pack(binding(), [], [], *pick(ok), seed=1)
    for need_dk in (True, False):
        numM, totdk = ev.debug_score_paths(h.host, need_dk=need_dk)
        vc.check_scores(h, numM, totdk, "k = %d, host-enumerated" % k, need_dk=need_dk)


@pytest.mark.parametrize("slots", [255, 256, 257])
def test_slot_totals_around_the_score_kernels_block(slots):
    """the score kernel runs 256 paths per block: 255, 256 and 257 slots, the last ones closed by the traverse kernel"""
    w, ix, ev = setup(21, True)
    idx, have = [], 0
    for i, (c, x) in enumerate(zip(w.clusters, w.scored)):
        pc = vc.caps_of(c, x)[0]
        if c.tag.startswith("random") and have + pc <= slots - 3:
            idx.append(i)
            have += pc
    b = vc.pack(binding(), [w.clusters[i] for i in idx], [w.scored[i] for i in idx], seed=slots, total_slots=slots)
    assert b.tables.path_cap == slots and (b.status == vc.OK).all()
    o = ev.debug_score_paths_trv(b.host, b.tables, need_dk=True)
    vc.check_traverse(b, o, "%d slots" % slots)
    vc.check_scores(b, o["numM"], o["totdk"], "%d slots" % slots)
    assert o["p_len"][-3:].tolist() == [0, 0, 0] and o["numM"][-3:].tolist() == [0, 0, 0] and o["totdk"][-3:].view(np.uint64).tolist() == [0, 0, 0]


def test_the_debug_entries_refuse_tables_that_point_outside():
    """nothing is launched on tables whose offsets leave their arrays, or whose path slots belong to no cluster"""
    import merfin_amd as m
    w, ix, ev = setup(21, True)
    b = vc.pack(binding(), w.clusters[:3], w.scored[:3])
    B = binding()
    t = B.TraverseTables(b.tables.cl.copy(), b.tables.var, b.tables.al, bytes(b.tables.win), bytes(b.tables.alt), b.tables.text_end, b.tables.path_cap + 1, b.tables.row_cap)
    with pytest.raises(m.MfxError):
        ev.debug_score_paths_trv(b.host, t)
    t = B.TraverseTables(b.tables.cl.copy(), b.tables.var, b.tables.al, bytes(b.tables.win), bytes(b.tables.alt), b.tables.text_end, b.tables.path_cap, b.tables.row_cap)
    t.cl[1]["path0"] = 0
    with pytest.raises(m.MfxError):
        ev.debug_score_paths_trv(b.host, t)
    with pytest.raises(m.MfxError):
        ev.debug_score_paths(B.PathTable(b"ACGT\n", [0], [9], [0], [0], [0]))


def test_host_form_on_a_used_scratch():
    """mfx_score_paths lays its batch out in the evaluator's scratch, as mfx_score_paths_trv does: on ONE evaluator the large
    device-enumerated batch, then host batches of ten clusters whose text is shorter than one 4096-byte tile (what the larger batch
    left behind their text and tables is still there), then a host batch whose text alone is longer than the whole first scratch (it
    has to be made again).  Every score bit for bit, with and without totdk."""
    import merfin_amd as m
    w, ix, _ = setup(21, True)
    ev = m.Evaluator(ix, m.KParams(vc.PEAK, w.probK, w.probP))          # its own evaluator: the scratch starts empty
    b = vc.pack(binding(), w.clusters, w.scored, seed=21)
    t = b.tables
    vc.check_scores(b, *[ev.debug_score_paths_trv(b.host, t, need_dk=True)[n] for n in ("numM", "totdk")], "the large batch first")
    # no more than the scratch it made: a quarter over the sum of its pieces (9 bytes per text byte and 3 tiles, 44 per slot, 12 per
    # row, the tables, 256 bytes of rounding for each of 21 pieces)
    scratch = 1.25 * (9 * t.text_end + 3 * 4096 + 256 + 44 * t.path_cap + 12 * t.row_cap + 16 + t.cl.nbytes + t.var.nbytes + t.al.nbytes
                      + len(t.win) + len(t.alt) + 8 * len(t.cl) + 21 * 256)
    ok = [i for i, x in enumerate(w.scored) if vc.status_of(w.clusters[i], x) == vc.OK]
    pick = lambda idx: ([w.clusters[i] for i in idx], [w.scored[i] for i in idx])
    size = lambda i: sum(len(p) + 1 for p in w.scored[i]["paths"])
    ten = lambda at: [i for i in ok[at:] if size(i) <= 400][:10]         # ten clusters from ok[at] on whose paths fit in one tile together
    for at in (0, len(ok) // 2, len(ok) - 40):
        h = vc.pack(binding(), [], [], *pick(ten(at)), seed=3)
        assert 0 < len(h.host.text) < 4096 and len(h.host.off) >= 10
        for need_dk in (True, False):
            vc.check_scores(h, *ev.debug_score_paths(h.host, need_dk=need_dk), "ten clusters from %d on a used scratch" % at, need_dk=need_dk)
    one = sum(map(size, ok))
    h = vc.pack(binding(), [], [], *pick(ok * (int(scratch) // one + 1)), seed=4)
    assert len(h.host.text) > scratch
    for need_dk in (True, False):
        vc.check_scores(h, *ev.debug_score_paths(h.host, need_dk=need_dk), "a host batch beyond the first scratch", need_dk=need_dk)
    h = vc.pack(binding(), [], [], *pick(ten(7)), seed=5)                   # and a short one again, on the grown scratch
    vc.check_scores(h, *ev.debug_score_paths(h.host), "ten clusters on the grown scratch")


def test_empty_calls_return_ok_and_write_nothing():
    """no path (npaths == 0) and no text (len == 0): MFX_OK from both debug entry points, numM / totdk as the caller filled them"""
    w, ix, ev = setup(21, True)
    B = binding()
    L = B.load_library()
    none = B.TraverseTables(np.zeros(0, dtype=B.TRV_CLUSTER_DTYPE), np.zeros(0, dtype=B.TRV_VARIANT_DTYPE), np.zeros(0, dtype=B.TRV_ALLELE_DTYPE), b"", b"", 0, 0, 0)
    for what, pt, text_end in (("npaths == 0", B.PathTable(b"ACGTACGTACGTACGTACGTACGTA\n"), 26), ("len == 0", B.PathTable(b"", [0, 0], [0, 0], [0, 0], [0, 0], [0, 1]), 0)):
        for need_dk in (1, 0):
            numM, totdk = np.full(4, 0xabcdabcd, dtype=np.uint32), np.full(4, -7.5)
            out = [need_dk, B.C.c_void_p(numM.ctypes.data), B.C.c_void_p(totdk.ctypes.data)]
            assert L.mfx_debug_score_paths(ev.h, *(pt.args() + out)) == 0, (what, L.mfx_last_error())
            none.text_end = text_end
            o, ptrs = B._trv_outputs(none)
            assert L.mfx_debug_score_paths_trv(ev.h, *(pt.args() + none.args() + out + ptrs)) == 0, (what, L.mfx_last_error())
            assert numM.tolist() == [0xabcdabcd] * 4 and totdk.tolist() == [-7.5] * 4, what
