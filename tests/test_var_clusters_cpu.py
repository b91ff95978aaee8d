"""The variant modes' traverse, cluster by cluster, without a GPU: mfx_debug_traverse_host (the scalar instantiation of
csrc/mfx_traverse.h -- the code the device runs one wave per cluster) against the oracle's traverse (oracle.pyoracle.cluster_paths:
merfin-variants.C:22-126 and varMer::addSeqPath restated with std::string) over the hand-written list and the seeded clusters of
tests/var_clusters.py: status, number of paths, text, '\\n' behind every path and everywhere nothing was reserved, path table,
genotype / offset / length rows.  A few clusters worked out by hand pin the oracle entry itself.  The rest asserts that the list
holds what it is meant to hold, so that tests/test_gpu_var_kernels.py (same clusters, on the device) tests what it claims."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import var_clusters as vc


def _binding():
    from merfin_amd import binding
    binding.load_library()
    return binding


# (window, variants, paths, gt rows, offset rows, length rows) -- worked out by hand from merfin-variants.C:22-126
LITERAL = [
    # one SNP
    (b"ACGTACGT", [(2, 1, [b"G", b"T"])], [b"ACGTACGT", b"ACTTACGT"], [[0], [1]], [[2], [2]], [[1], [1]]),
    # an insertion shifts the later variant's offset (5 -> 7) while it is in place, and its own length becomes the ALT's
    (b"AACCGGTT", [(2, 1, [b"C", b"CTT"]), (5, 1, [b"G", b"A"])], [b"AACCGGTT", b"AACCGATT", b"AACTTCGGTT", b"AACTTCGATT"],
     [[0, 0], [0, 1], [1, 0], [1, 1]], [[2, 5], [2, 5], [2, 7], [2, 7]], [[1, 1], [1, 1], [3, 1], [3, 1]]),
    # the second variant starts inside the first one's REF span: forced to REF, and as it is the last one the path is added at once
    # (offsets not shifted)
    (b"ACGTACGTAC", [(2, 3, [b"GTA", b"G"]), (3, 1, [b"T", b"C"])], [b"ACGTACGTAC", b"ACGCACGTAC", b"ACGCGTAC"],
     [[0, 0], [0, 1], [1, 0]], [[2, 3], [2, 3], [2, 3]], [[3, 1], [3, 1], [1, 1]]),
    # deleting either of two equal bases gives the same sequence: added once, with the rows of the first way
    (b"CAAT", [(1, 1, [b"A", b""]), (2, 1, [b"A", b""])], [b"CAAT", b"CAT", b"CT"], [[0, 0], [0, 1], [1, 1]], [[1, 2], [1, 2], [1, 1]],
     [[1, 1], [1, 0], [0, 0]]),
    # an insertion at the very end (pos == size is legal for std::string::replace), REF length clipped to nothing
    (b"ACG", [(3, 2, [b"", b"TT"])], [b"ACG", b"ACGTT"], [[0], [1]], [[3], [3]], [[2], [2]]),
]


def test_hand_worked_clusters_pin_oracle_and_host_traverse():
    binding = _binding()
    cls, res = [], []
    for i, (win, variants, paths, gt, vidx, vlen) in enumerate(LITERAL):
        c = vc.Cluster("literal_%d" % i, win, variants)
        x = vc.traverse_oracle(c)
        assert x["status"] == 0 and x["paths"] == paths, (i, x["paths"])
        assert x["gt"].tolist() == gt and x["vidx"].tolist() == vidx and x["vlen"].tolist() == vlen, (i, x)
        assert x["longest"] == max(len(p) for p in paths)
        cls.append(c)
        res.append(x)
    b = vc.pack(binding, cls, res, seed=3)
    o = binding.debug_traverse_host(b.tables)
    vc.check_traverse(b, o, "literal")
    # and directly, not through the packer's expectation: the last cluster's rows and text as the device part holds them
    c = b.tables.cl[-1]
    t0, p0, r0 = int(c["text0"]), int(c["path0"]), int(c["row0"])
    assert bytes(o["text"][t0:t0 + 10]) == b"ACG\nACGTT\n" and o["p_len"][p0:p0 + 2].tolist() == [3, 5]
    assert o["gt"][r0:r0 + 2].tolist() == [0, 1] and o["vidx"][r0:r0 + 2].tolist() == [3, 3] and o["vlen"][r0:r0 + 2].tolist() == [2, 2]
    assert o["p_cfirst"][p0:p0 + 2].tolist() == [p0, p0] and o["p_voff"][p0:p0 + 2].tolist() == [r0, r0 + 1]
    # std::string::replace throws past the end: the oracle reports it
    x = vc.traverse_oracle(vc.Cluster("range", b"ACG", [(4, 0, [b"", b"T"])]))
    assert x["status"] == 1 and x["paths"] == [b"ACG"]


@pytest.mark.parametrize("k", [21, 22, 31, 33, 64])
def test_host_traverse_equals_oracle(k):
    binding = _binding()
    cls = vc.hand_clusters(k) + vc.random_clusters(k, 900 + k, 1500)
    res = [vc.traverse_oracle(c) for c in cls]
    b = vc.pack(binding, cls, res, seed=k)
    for c, st in zip(cls, b.status):
        assert st == c.expect, (c.tag, st, c.expect)
    assert sorted(set(b.status.tolist())) == [vc.OK, vc.RANGE, vc.ROOM]
    o = binding.debug_traverse_host(b.tables)
    vc.check_traverse(b, o, "k = %d" % k)
    # every path is followed by '\n' (read directly from the returned table)
    used = o["p_len"] > 0
    assert (o["text"][(o["p_off"] + o["p_len"])[used & b.slot_care].astype(np.int64)] == 10).all()
    # the same clusters in another order and with a host part in front: text0 / path0 / row0 are the caller's
    order = np.random.default_rng(k).permutation(len(cls))
    b2 = vc.pack(binding, [cls[i] for i in order], [res[i] for i in order], seed=k + 1)
    vc.check_traverse(b2, binding.debug_traverse_host(b2.tables), "k = %d, permuted" % k)


def test_tables_are_checked_before_anything_runs():
    binding = _binding()
    c = vc.Cluster("x", b"ACGTACGT", [(2, 1, [b"G", b"T"])])
    b = vc.pack(binding, [c], [vc.traverse_oracle(c)])
    for field, value in (("win_len", 9000), ("var0", 5), ("text_cap", 9000), ("path0", 7), ("row0", 100), ("text0", 2**40)):
        t = binding.TraverseTables(b.tables.cl.copy(), b.tables.var, b.tables.al, bytes(b.tables.win), bytes(b.tables.alt), b.tables.text_end,
                                   b.tables.path_cap, b.tables.row_cap)
        t.cl[0][field] = value
        with pytest.raises(binding.MfxError):
            binding.debug_traverse_host(t)
    for arr, field in (("var", "al0"), ("al", "off"), ("al", "len")):
        t = binding.TraverseTables(b.tables.cl, b.tables.var.copy(), b.tables.al.copy(), bytes(b.tables.win), bytes(b.tables.alt), b.tables.text_end,
                                   b.tables.path_cap, b.tables.row_cap)
        getattr(t, arr)[0][field] = 1000
        with pytest.raises(binding.MfxError):
            binding.debug_traverse_host(t)


@pytest.mark.parametrize("k", [21, 64])
def test_the_list_holds_what_it_names(k):
    """every listed edge is there and has the effect it is there for (from the oracle's results)"""
    cls = vc.hand_clusters(k)
    by = {c.tag: (c, vc.traverse_oracle(c)) for c in cls}
    assert len(by) == len(cls)
    n_paths = lambda t: len(by[t][1]["paths"])
    for nv in range(1, 9):
        assert by["nv%d" % nv][0].nv == nv and n_paths("nv%d" % nv) == 2**nv
    assert [n_paths("na%d" % a) for a in (2, 3, 4)] == [4, 9, 16]
    assert n_paths("product64_six") == 64 and by["product64_six"][0].nv == 6 and n_paths("product64_444") == 64 and n_paths("mixed_234") == 24
    assert by["nv9"][0].nv == 9
    assert len(by["win640"][0].win) == 640 and len(by["win641"][0].win) == 641
    assert by["ins_to_641"][1]["longest"] == 641 and by["ins_to_640"][1]["longest"] == 640 and by["ins_to_641_second"][1]["longest"] == 641
    assert len(by["ins_to_641_second"][0].win) + 4 <= 640
    assert by["pos_past_end"][1]["status"] == 1 and by["pos_past_end_second"][1]["status"] == 1 and by["pos_at_end"][1]["status"] == 0
    assert by["pos_at_end"][1]["paths"][1] == by["pos_at_end"][0].win + b"ACG"
    assert by["reflen_clipped"][1]["paths"][1] == by["reflen_clipped"][0].win[:-2] + b"T" and by["reflen_clipped"][1]["vlen"].tolist() == [[5], [1]]
    assert by["allele_len0"][1]["vlen"].tolist() == [[2], [0]]
    x = by["long_ins_del"][1]
    assert n_paths("long_ins_del") == 12 and len({tuple(r) for r in x["vidx"].tolist()}) >= 6 and x["vidx"][0].tolist() == x["vidx"][1].tolist()[:2] + [x["vidx"][0][2]]
    assert max(len(p) for p in x["paths"]) - min(len(p) for p in x["paths"]) > 300
    # overlaps: the skipped variants are REF on every path whose earlier variant is ALT
    assert by["skip_one"][1]["gt"].tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1]]
    assert [g for g in by["skip_two"][1]["gt"].tolist() if g[0] == 1] == [[1, 0, 0, 0], [1, 0, 0, 1]]
    assert by["skip_last"][1]["gt"].tolist() == [[0, 0], [0, 1], [1, 0], [2, 0]]
    assert [g for g in by["skip_two_last"][1]["gt"].tolist() if g[1] == 1] == [[0, 1, 0, 0], [1, 1, 0, 0]]
    assert [g for g in by["same_offset"][1]["gt"].tolist() if g[0] == 1] == [[1, 0, 0], [1, 0, 1]]
    # duplicates dropped, near-duplicates kept
    assert n_paths("dup_alt_is_ref") == 2 < by["dup_alt_is_ref"][0].product and n_paths("dup_two_ways") == 3
    for n in (63, 64, 65, 128, 129, 600):
        for at in (0, 63, 64, 65, 127, 128, n - 1):
            if at < n:
                a, b = by["near_%d_%d" % (n, at)][1]["paths"]
                assert len(a) == len(b) == n and [i for i in range(n) if a[i] != b[i]] == [at]
        assert n_paths("near3_%d" % n) == 4
    # bytes
    seen = set()
    for c in cls:
        seen |= set(c.win)
        for v in c.variants:
            for a in v[2]:
                seen |= set(a)
    assert seen == set(range(256)) - {0, 10}
    low = by["lower_and_n"][0].win
    assert any(ch in low for ch in b"acgt") and b"NNN" in low and b"n" in low
    if k % 2 == 0:
        w = by["palindrome"][0].win[k - 1:2 * k - 1].decode()
        assert w == "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[ch] for ch in reversed(w))
    # score: path lengths around k, offsets around k - 1, the last index of the bump window
    assert sorted(len(p) for p in by["short_paths"][1]["paths"]) == [k - 1, k + 1, k + 2]
    assert sorted(len(p) for p in by["exactly_k"][1]["paths"]) == [k - 1, k, k]
    assert by["off_0"][0].variants[0][0] == 0 and by["off_k_minus_2"][0].variants[0][0] == k - 2 and by["off_k_minus_1"][0].variants[0][0] == k - 1
    for vl in (0, 1, 3):
        for extra in (0, 1, 2):
            x = by["bump_end_vl%d_x%d" % (vl, extra)][1]
            assert x["gt"].tolist() == [[0], [1]] and x["vlen"][1].tolist() == [vl]
            assert len(x["paths"][1]) - 1 == int(x["vidx"][1][0]) + vl + k - 1 + extra      # the ALT path's last index
    x = by["two_windows"][1]
    assert any(g[0] > 0 and g[1] > 0 and abs(int(a[0]) - int(a[1])) < k for g, a in zip(x["gt"].tolist(), x["vidx"].tolist()))
    assert {g for row in by["alleles_2_3"][1]["gt"].tolist() for g in row} == {0, 1, 2, 3}
    assert b"N" in by["n_in_bump"][0].win[k - 1:2 * k]
    valid = lambda p: any(all(ch in b"ACGTacgt" for ch in p[i:i + k]) for i in range(len(p) - k + 1))
    for t in ("look_back_two_n", "look_back_two_short"):
        v = [valid(p) for p in by[t][1]["paths"]]
        assert any(v[i] and not v[i + 1] and i + 2 < len(v) for i in range(len(v) - 1)), (t, v)     # a path whose predecessor has no k-mer
    assert not any(valid(p) for p in by["all_n"][1]["paths"][:1])


@pytest.mark.parametrize("k,use_prob", [(21, True), (22, False)])
def test_every_count_class_occurs(k, use_prob):
    w = vc.world(k, use_prob, 200)
    assert w.read_classes == set(vc.READ_PALETTE) and w.asm_classes == set(vc.ASM_PALETTE)
    assert vc.READ_PALETTE["half_1"] / vc.PEAK == 1.5 and vc.READ_PALETTE["half_2"] / vc.PEAK == 2.5 and vc.READ_PALETTE["half_5"] / vc.PEAK == 5.5
    assert vc.READ_PALETTE["below_peak"] < vc.PEAK == vc.READ_PALETTE["peak"]
    assert 0.0 in vc.PROB_P and 1.0 in vc.PROB_P and any(0 < p < 1 for p in vc.PROB_P)
    # the scores feel them: totdk takes many values, with -prob also fractions of the table's probabilities
    tot = np.concatenate([x["totdk"] for x in w.scored])
    num = np.concatenate([x["numM"] for x in w.scored])
    assert len(set(tot.tolist())) > 50 and num.max() > 0 and (num == 0).any()
    if use_prob:
        assert (tot != np.round(tot)).any()
    # and the oracle agrees with itself: -filter's numM is the same count
    c = w.clusters[0]
    assert po.cluster_paths(w.params, None, None, c.win, c.variants, need_dk=False, cb=po.getk_text_fn(lambda t: (0.0, 0.0, 1.0)))["totdk"].tolist() == [0.0, 0.0]
