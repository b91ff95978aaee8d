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
