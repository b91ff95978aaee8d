"""Variant clusters for the tests of the traverse and score kernels (tests/test_var_clusters_cpu.py, tests/test_gpu_var_kernels.py):
a hand-written list of the edges of csrc/mfx_traverse.h and mfx_var_score_kernel, seeded random clusters, the packer that lays a
batch out as the tables the device reads, and what the oracle (oracle.pyoracle.cluster_paths: the reference's traverse and
varMer::score, one cluster in, every path out) says the batch must come back as.

A helper like tests/kstar_grid.py: no test in here.  Everything is deterministic (seeded), and nothing here needs a GPU."""
import functools

import numpy as np

from oracle import plain
from oracle import pyoracle as po

MAX_NV, MAX_LEN = 8, 640
OK, RANGE, ROOM = 0, 1, 2
PEAK = 20.0
# -prob table: row i is read count i + 1 -> (readK, prob); probabilities 0.0, 1.0 and values between
PROB_K = [1, 1, 2, 1, 3, 1, 2, 1]
PROB_P = [0.0, 1.0, 0.25, 0.5, 0.75, 0.125, 1.0, 0.3]
N_PROB = len(PROB_K)
# read counts: absent, 1, just below / at peak, readV / peak = n + 0.5 (round() half away from zero), the last row of the -prob table and the
# first count behind it, 16- and 32-bit ends (the other table rows make the carried prob vary)
READ_PALETTE = {"absent": 0, "one": 1, "below_peak": 19, "peak": 20, "half_1": 30, "half_2": 50, "half_5": 110, "n_prob": N_PROB,
                "n_prob_plus_1": N_PROB + 1, "u16": 65535, "u32": 2**32 - 1, "row2": 2, "row3": 3, "row4": 4, "row5": 5, "row6": 6}
ASM_PALETTE = {"absent": 0, "one": 1, "two": 2, "large": 100000}


class Cluster:
    """win: the window's bytes; variants: [(offset, REF length, [alleles, REF first])]; path_cap / text_cap: None = what the cluster
    needs (the product of the allele counts / the bytes of its paths) plus `slack`; expect: the status the tables must give"""

    def __init__(self, tag, win, variants, path_cap=None, text_cap=None, slack=(0, 0), expect=OK):
        self.tag, self.win, self.variants = tag, bytes(win), [(int(o), int(r), [bytes(a) for a in al]) for o, r, al in variants]
        self.path_cap, self.text_cap, self.slack, self.expect = path_cap, text_cap, slack, expect

    @property
    def nv(self):
        return len(self.variants)

    @property
    def product(self):
        n = 1
        for v in self.variants:
            n *= len(v[2])
        return n


def _bases(r, n):
    return bytes(r.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


def _other(b, step=1):
    return b"ACGT"[(b"ACGT".index(bytes([b]).upper()) + step) % 4:][:1]


def _snps(r, win, offs, na=2):
    return [(o, 1, [win[o:o + 1]] + [_other(win[o], s) for s in range(1, na)]) for o in offs]


def hand_clusters(k):
    """the listed edges; tags are what test_var_clusters_cpu.py asserts the presence (and the effect) of"""
    r = np.random.default_rng(1000 + k)
    L = []
    add = lambda *a, **kw: L.append(Cluster(*a, **kw))
    pad = k - 1
    # ---- traverse: nv = 1 .. 8 (biallelic, 3 apart), allele counts 2 .. 4
    for nv in range(1, 9):
        w = _bases(r, 2 * pad + 3 * nv)
        add("nv%d" % nv, w, _snps(r, w, [pad + 3 * i for i in range(nv)]))
    for na in (2, 3, 4):
        w = _bases(r, 2 * pad + 8)
        add("na%d" % na, w, _snps(r, w, [pad, pad + 5], na))
    w = _bases(r, 2 * pad + 30)
    add("product64_six", w, _snps(r, w, [pad + 4 * i for i in range(6)]))
    w = _bases(r, 2 * pad + 12)
    add("product64_444", w, _snps(r, w, [pad, pad + 4, pad + 8], 4))
    w = _bases(r, 2 * pad + 9)
    add("mixed_234", w, [_snps(r, w, [pad], 2)[0], _snps(r, w, [pad + 3], 3)[0], _snps(r, w, [pad + 6], 4)[0]])
    # ---- room
    w = _bases(r, 2 * pad + 6)
    add("room_paths", w, _snps(r, w, [pad, pad + 3]), path_cap=3, expect=ROOM)
    add("room_text", w, _snps(r, w, [pad, pad + 3]), text_cap=4 * (len(w) + 1) - 1, expect=ROOM)
    add("room_exact", w, _snps(r, w, [pad, pad + 3]), path_cap=4, text_cap=4 * (len(w) + 1))
    w = _bases(r, 40)
    add("nv9", w, _snps(r, w, [3 * i + 2 for i in range(9)]), path_cap=2, text_cap=2 * 41, expect=ROOM)
    w = _bases(r, 640)
    add("win640", w, _snps(r, w, [300]))
    w = _bases(r, 641)
    add("win641", w, _snps(r, w, [300]), expect=ROOM)
    w = _bases(r, 640)
    add("ins_to_641", w, [(100, 1, [w[100:101], w[100:101] + b"G"])], expect=ROOM)
    w = _bases(r, 639)
    add("ins_to_640", w, [(100, 1, [w[100:101], w[100:101] + b"G"])])
    w = _bases(r, 636)
    add("ins_to_641_second", w, [(100, 1, [w[100:101], w[100:101] + b"GTAC"]), (200, 1, [w[200:201], w[200:201] + b"T"])], expect=ROOM)
    # ---- replacement position and clipped lengths
    w = _bases(r, 2 * pad + 5)
    add("pos_at_end", w, [(len(w), 0, [b"", b"ACG"])])
    add("pos_past_end", w, [(len(w) + 1, 0, [b"", b"ACG"])], expect=RANGE)
    add("pos_past_end_second", w, [(pad, 1, [w[pad:pad + 1], _other(w[pad])]), (len(w) + 1, 1, [b"A", b"C"])], expect=RANGE)
    add("reflen_clipped", w, [(len(w) - 2, 5, [w[-2:] + b"AAA", b"T"])])
    add("reflen_clipped_at_end", w, [(len(w), 4, [b"ACGT", b"TT"])])
    add("allele_len0", w, [(pad, 2, [w[pad:pad + 2], b""])])
    add("allele_len0_ref", w, [(pad, 0, [b"", b"GG"]), (pad + 3, 1, [w[pad + 3:pad + 4], b""])])
    # ---- long insertions / deletions: later offsets shift and are restored
    w = _bases(r, 2 * pad + 260)
    add("long_ins_del", w, [(pad, 1, [w[pad:pad + 1], _bases(r, 150)]), (pad + 20, 200, [w[pad + 20:pad + 220], b"A", _bases(r, 37)]),
                            (pad + 240, 2, [w[pad + 240:pad + 242], _bases(r, 60)])])
    w = _bases(r, 400)
    add("long_del_first", w, [(10, 300, [w[10:310], b""]), (350, 1, [w[350:351], _bases(r, 99)]), (380, 1, [w[380:381], b"NN"])])
    # ---- overlaps: a later variant starts inside the REF span just replaced
    w = _bases(r, 2 * pad + 40)
    p = pad
    add("skip_one", w, [(p, 5, [w[p:p + 5], b"G"]), (p + 2, 1, [w[p + 2:p + 3], b"TT"]), (p + 20, 1, [w[p + 20:p + 21], b"CA"])])
    add("skip_two", w, [(p, 10, [w[p:p + 10], b"GA"]), (p + 2, 1, [w[p + 2:p + 3], b"T"]), (p + 6, 2, [w[p + 6:p + 8], b"C"]),
                        (p + 30, 1, [w[p + 30:p + 31], b"ACGT"])])
    add("skip_last", w, [(p, 5, [w[p:p + 5], b"G", b"TTTTTTT"]), (p + 2, 1, [w[p + 2:p + 3], b"TT"])])
    add("skip_two_last", w, [(p, 1, [w[p:p + 1], b"GG"]), (p + 4, 9, [w[p + 4:p + 13], b""]), (p + 5, 1, [w[p + 5:p + 6], b"A"]), (p + 12, 1, [w[p + 12:p + 13], b"C"])])
    add("same_offset", w, [(p, 1, [w[p:p + 1], _other(w[p])]), (p, 1, [w[p:p + 1], _other(w[p], 2)]), (p + 9, 1, [w[p + 9:p + 10], b"AC"])])
    # ---- duplicates that addSeqPath drops
    add("dup_alt_is_ref", w, [(p, 2, [w[p:p + 2], w[p:p + 2], _other(w[p]) + w[p + 1:p + 2]]), (p + 8, 1, [w[p + 8:p + 9], w[p + 8:p + 9]])])
    w2 = w[:p] + b"AA" + w[p + 2:]
    add("dup_two_ways", w2, [(p, 1, [b"A", b""]), (p + 1, 1, [b"A", b""])])
    # ---- near-duplicates it must keep: equal length, ONE differing byte at index at
    for n in (63, 64, 65, 128, 129, 600):
        w = _bases(r, n)
        for at in sorted({0, 63, 64, 65, 127, 128, n - 1}):
            if at < n:
                add("near_%d_%d" % (n, at), w, _snps(r, w, [at]))
        add("near3_%d" % n, w, _snps(r, w, [n - 1], 4))                    # later paths compared against several of equal length
    # ---- bytes: lower case, N runs, every byte value except NUL and '\n'
    junk = [b for b in range(1, 256) if b != 10]
    per = max(1, 560 // (k + 6))
    for i in range(0, len(junk), per):
        w = b"".join(_bases(r, int(r.integers(k, k + 5))) + bytes([b]) for b in junk[i:i + per]) + _bases(r, k + 1)
        at = k + 2 if len(w) > k + 3 else 0
        add("bytes_%d" % i, w, [(at, 1, [w[at:at + 1], b"g", bytes([junk[i]])])])
    w = _bases(r, 2 * pad + 30)
    w = w[:5].lower() + w[5:pad + 8] + b"NNN" + w[pad + 11:pad + 20].lower() + b"n" + w[pad + 21:]
    add("lower_and_n", w, [(pad, 1, [w[pad:pad + 1], b"t"]), (pad + 9, 1, [b"N", b"a", b"NN"]), (pad + 15, 2, [w[pad + 15:pad + 17], b"c"])])
    h = _bases(r, k // 2)
    pal = h + plain.revcomp(h.decode()).encode()
    w = _bases(r, pad) + pal + _bases(r, pad + 2)
    add("palindrome", w, [(pad + 1, 1, [w[pad + 1:pad + 2], b"AA"])])
    # ---- score: the bump window idxPath + 1 - k <= idx < idxPath + lenPath + k (uint32), prob carry
    w = _bases(r, 3 * k + 10)
    add("short_paths", w[:k + 1], [(2, 2, [w[2:4], b"", b"GTA"])])             # k - 1, k + 1 and k + 2 bases
    add("exactly_k", w[:k], [(k // 2, 1, [w[k // 2:k // 2 + 1], _other(w[k // 2]), b""])])
    add("off_0", w, [(0, 1, [w[0:1], _other(w[0]), b"GG"])])                       # offset < k - 1: the wrap, no bump at all
    add("off_k_minus_2", w, [(k - 2, 1, [w[k - 2:k - 1], _other(w[k - 2]), b"GG"])])
    add("off_k_minus_1", w, [(k - 1, 1, [w[k - 1:k], _other(w[k - 1]), b"GG", b""])])
    for vl, alt in ((0, b""), (1, b"T"), (3, b"TGC")):                       # ALT path: vi = k + 4, vi + vl + k + extra bases -- its last index is the
        for extra in (0, 1, 2):                                                # window's last (extra 0), or one / two behind it
            ww = w[:k + 4] + b"A" + w[k + 5:2 * k + 5 + extra]
            add("bump_end_vl%d_x%d" % (vl, extra), ww, [(k + 4, 1, [b"A", alt])])
    add("two_windows", w, [(k, 1, [w[k:k + 1], _other(w[k])]), (k + 3, 1, [w[k + 3:k + 4], _other(w[k + 3]), b"AAC"])])
    add("alleles_2_3", w, _snps(r, w, [k - 1, k + 7], 4))
    wn = w[:k + 2] + b"N" + w[k + 3:]
    add("n_in_bump", wn, [(k - 1, 1, [wn[k - 1:k], _other(wn[k - 1]), b"NNN"]), (k + 6, 1, [wn[k + 6:k + 7], b"n"])])
    ws = w[:2 * k - 1]
    add("look_back_two_n", ws, [(k - 1, 1, [ws[k - 1:k], b"N", _other(ws[k - 1]), b"n", b"CG"])])     # paths 2 and 4 have no k-mer at all
    add("look_back_two_short", w[:k + 1], [(k - 1, 1, [w[k - 1:k], b"", b"GT", b"", b"TTT"]), (k, 1, [w[k:k + 1], b"", b"A"])])
    add("all_n", b"N" * (2 * k), [(k - 1, 1, [b"N", b"A", b"NN"])])
    return L


def random_clusters(k, seed, n):
    """clusters shaped like a call set's (windows padded by k - 1 on either side, variants in order, some overlapping), alleles of 0 .. 12
    bases, a few lower-case bases and Ns, products of at most 64, room with and without slack"""
    r = np.random.default_rng(seed)
    out = []
    for c in range(n):
        nv = int(r.choice([1, 1, 2, 2, 3, 4, 5, 6]))
        nas = [int(r.choice([2, 2, 2, 3, 4])) for _ in range(nv)]
        while np.prod(nas) > 64:
            nas[int(np.argmax(nas))] -= 1
        gaps = r.integers(0, 9, size=nv)
        offs, o = [], k - 1
        for g in gaps:
            o += int(g)
            offs.append(o)
            o += 1
        w = bytearray(_bases(r, offs[-1] + 6 + k - 1))
        for _ in range(int(r.integers(0, 3))):
            i = int(r.integers(0, len(w)))
            w[i] = ord("N") if r.random() < 0.4 else w[i] | 0x20
        w = bytes(w)
        vs = []
        for o, na in zip(offs, nas):
            rl = int(r.choice([1, 1, 1, 2, 4, 0]))
            rl = min(rl, len(w) - o)
            als = [w[o:o + rl]]
            for _ in range(na - 1):
                a = _bases(r, int(r.choice([0, 1, 1, 1, 2, 3, 5, 12])))
                if r.random() < 0.1:
                    a = a.lower()
                als.append(a)
            vs.append((o, rl, als))
        slack = (int(r.choice([0, 0, 1, 3])), int(r.choice([0, 0, 1, 7])))
        out.append(Cluster("random_%d" % c, w, vs, slack=slack))
    return out


EMPTY = None


def traverse_oracle(cl):
    """traverse alone (k plays no part in it): the oracle's paths of a cluster, unscored"""
    global EMPTY
    if EMPTY is None:
        EMPTY = (po.Params(21, PEAK), po.Lookup(21, [], []), po.Lookup(21, [], []))
    return po.cluster_paths(EMPTY[0], EMPTY[1], EMPTY[2], cl.win, cl.variants, need_dk=False)


def need_of(cl, res):
    """(paths, text bytes) the cluster's result takes"""
    return len(res["paths"]), sum(len(p) + 1 for p in res["paths"])


def caps_of(cl, res):
    n, t = need_of(cl, res)
    pc = cl.path_cap if cl.path_cap is not None else max(cl.product, n if res["status"] == 0 else 0) + cl.slack[0]
    tc = cl.text_cap if cl.text_cap is not None else t + cl.slack[1]
    return pc, tc


def status_of(cl, res):
    """the status the device must report, from the oracle's result and the caps"""
    pc, tc = caps_of(cl, res)
    n, t = need_of(cl, res)
    causes = []
    if res["status"]:
        causes.append(RANGE)
    if cl.nv > MAX_NV:
        causes.append(ROOM)
    if len(cl.win) > MAX_LEN:
        causes.append(ROOM)
    if len(cl.win) <= MAX_LEN and res["longest"] > MAX_LEN:
        causes.append(ROOM)
    if not res["status"] and cl.nv <= MAX_NV and res["longest"] <= MAX_LEN and (n > pc or t > tc):
        causes.append(ROOM)
    assert len(causes) <= 1, (cl.tag, causes)               # a faulting cluster has ONE cause
    return causes[0] if causes else OK


class Batch:
    """clusters laid out for the device: `tables` (merfin_amd.binding.TraverseTables), the host part `host` (PathTable), and what must
    come back -- arrays of the device part plus `care` masks (False where a faulting cluster may have written what it likes)"""


def pack(binding, clusters, results, host=(), host_results=(), seed=0, total_slots=None):
    """host / host_results: clusters whose oracle paths go in front as the HOST-enumerated part (their status must be OK).
    total_slots: the device part's path slots are brought to exactly this number by widening the last cluster's room."""
    r = np.random.default_rng(seed)
    b = Batch()
    # ---- host part
    ht, off, plen, nvs, voff, cfirst, gt, vidx, vlen, h_numM, h_totdk = bytearray(), [], [], [], [], [], [], [], [], [], []
    for cl, res in zip(host, host_results):
        assert res["status"] == 0
        first = len(off)
        for i, p in enumerate(res["paths"]):
            off.append(len(ht)); plen.append(len(p)); nvs.append(cl.nv); voff.append(len(gt)); cfirst.append(first)
            ht += p + b"\n"
            gt += res["gt"][i].tolist(); vidx += res["vidx"][i].tolist(); vlen += res["vlen"][i].tolist()
        if "numM" in res:
            h_numM += res["numM"].tolist(); h_totdk += res["totdk"].tolist()
    b.host = binding.PathTable(ht, off, plen, nvs, voff, cfirst, gt, vidx, vlen)
    hp, hv, hl = len(off), len(gt), len(ht)
    # ---- device part
    ncl = len(clusters)
    cls = np.zeros(ncl, dtype=binding.TRV_CLUSTER_DTYPE)
    var, al, win, alt = [], [], bytearray(), bytearray()
    caps = [list(caps_of(c, x)) for c, x in zip(clusters, results)]
    if total_slots is not None:
        have = sum(c[0] for c in caps)
        assert total_slots >= have
        caps[-1][0] += total_slots - have
    text_at, path_at, row_at = hl, 0, 0
    for i, (cl, res) in enumerate(zip(clusters, results)):
        text_at += int(r.integers(0, 4))                     # room nobody reserved, between the clusters
        win += b"\x07" * int(r.integers(0, 3))
        cls[i] = (len(win), len(cl.win), cl.nv, len(var), caps[i][0], text_at, path_at, row_at, caps[i][1], 0)
        win += cl.win
        for o, rl, als in cl.variants:
            var.append((o, rl, len(als), len(al)))
            for a in als:
                al.append((len(alt), len(a), 0))
                alt += a + b"\x07"
        text_at += caps[i][1]
        path_at += caps[i][0]
        row_at += caps[i][0] * cl.nv
    text_end = text_at + int(r.integers(0, 4))
    b.tables = binding.TraverseTables(cls, np.array(var, dtype=binding.TRV_VARIANT_DTYPE), np.array(al, dtype=binding.TRV_ALLELE_DTYPE), win, alt,
                                      text_end, path_at, row_at)
    # ---- what must come back
    b.status = np.array([status_of(c, x) for c, x in zip(clusters, results)], dtype=np.uint32)
    b.np = np.array([len(x["paths"]) for x in results], dtype=np.uint32)
    b.text = np.full(text_end, 10, dtype=np.uint8)
    b.text[:hl] = np.frombuffer(bytes(ht), dtype=np.uint8)
    b.text_care = np.ones(text_end, dtype=bool)
    P, R = path_at, row_at
    b.p_off, b.p_len, b.p_nv = np.zeros(P, dtype=np.uint64), np.zeros(P, dtype=np.uint32), np.zeros(P, dtype=np.uint32)
    b.p_voff, b.p_cfirst = np.zeros(P, dtype=np.uint64), np.zeros(P, dtype=np.uint64)
    b.slot_care = np.ones(P, dtype=bool)
    b.gt, b.vidx, b.vlen = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.uint32), np.zeros(R, dtype=np.uint32)
    b.row_care = np.zeros(R, dtype=bool)                     # (rows of unused slots are never written: whatever the buffer held)
    b.numM = np.zeros(hp + P, dtype=np.uint32)
    b.totdk = np.zeros(hp + P, dtype=np.float64)
    b.numM[:hp] = h_numM if h_numM else 0
    b.totdk[:hp] = h_totdk if h_totdk else 0.0
    b.hp, b.hv = hp, hv
    for i, (cl, res) in enumerate(zip(clusters, results)):
        c = cls[i]
        t0, p0, r0, pc, tc = int(c["text0"]), int(c["path0"]), int(c["row0"]), int(c["path_cap"]), int(c["text_cap"])
        if b.status[i] != OK:
            b.text_care[t0:t0 + tc] = False
            b.slot_care[p0:p0 + pc] = False
            continue
        at = t0
        for j, p in enumerate(res["paths"]):
            b.text[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
            b.p_off[p0 + j], b.p_len[p0 + j], b.p_nv[p0 + j] = at, len(p), cl.nv
            b.p_voff[p0 + j], b.p_cfirst[p0 + j] = hv + r0 + j * cl.nv, hp + p0
            rr = slice(r0 + j * cl.nv, r0 + (j + 1) * cl.nv)
            b.gt[rr], b.vidx[rr], b.vlen[rr], b.row_care[rr] = res["gt"][j], res["vidx"][j], res["vlen"][j], True
            at += len(p) + 1
        for q in range(p0 + len(res["paths"]), p0 + pc):      # closed slots
            b.p_off[q], b.p_cfirst[q] = t0, hp + q
        if "numM" in res:
            n = len(res["paths"])
            b.numM[hp + p0:hp + p0 + n], b.totdk[hp + p0:hp + p0 + n] = res["numM"], res["totdk"]
    b.score_care = np.concatenate([np.ones(hp, dtype=bool), b.slot_care])
    return b


def check_traverse(b, o, where):
    """the device part of a result dict (binding.debug_traverse_host / Evaluator.debug_score_paths_trv) against the batch's expectation"""
    assert o["status"].tolist() == b.status.tolist(), where
    ok = b.status == OK
    assert o["np"][ok].tolist() == b.np[ok].tolist(), where
    bad = np.flatnonzero((o["text"] != b.text) & b.text_care)
    assert bad.size == 0, (where, "text differs at byte", int(bad[0]), bytes(o["text"][max(0, int(bad[0]) - 20):int(bad[0]) + 20]), bytes(b.text[max(0, int(bad[0]) - 20):int(bad[0]) + 20]))
    for name in ("p_off", "p_len", "p_nv", "p_voff", "p_cfirst"):
        bad = np.flatnonzero((o[name] != getattr(b, name)) & b.slot_care)
        assert bad.size == 0, (where, name, "slot", int(bad[0]), int(o[name][bad[0]]), int(getattr(b, name)[bad[0]]))
    for name in ("gt", "vidx", "vlen"):
        bad = np.flatnonzero((o[name] != getattr(b, name)) & b.row_care)
        assert bad.size == 0, (where, name, "row", int(bad[0]), int(o[name][bad[0]]), int(getattr(b, name)[bad[0]]))


def check_scores(b, numM, totdk, where, need_dk=True):
    """numM equal, totdk equal as BIT PATTERNS, over the host part and every slot of the OK clusters (closed slots: 0 / +0.0)"""
    bad = np.flatnonzero((numM != b.numM) & b.score_care)
    assert bad.size == 0, (where, "numM: %d paths differ; first" % bad.size, int(bad[0]), int(numM[bad[0]]), int(b.numM[bad[0]]))
    if need_dk:
        bad = np.flatnonzero((totdk.view(np.uint64) != b.totdk.view(np.uint64)) & b.score_care)
        assert bad.size == 0, (where, "totdk: %d paths differ; first" % bad.size, int(bad[0]), float(totdk[bad[0]]), float(b.totdk[bad[0]]),
                               "largest difference %g" % np.nanmax(np.abs(totdk[bad] - b.totdk[bad])))


# ---------------------------------------------------------------------------------------------------------------------------------
# counts: every canonical k-mer of the oracle's path texts gets a read and an assembly count from the palettes
# ---------------------------------------------------------------------------------------------------------------------------------
_DIGIT = bytes.maketrans(b"ACTGactg", b"01230123")
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")


def canonical_kmers(k, texts):
    """the distinct canonical k-mers (Python ints, meryl's encoding A C T G = 0 1 2 3) of byte strings; a k-mer is k bases ACGT, either case"""
    seen, out = set(), set()
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGTacgt")] = True
    for t in texts:
        if len(t) < k:
            continue
        bad = np.concatenate([[0], np.cumsum(~ok[np.frombuffer(t, dtype=np.uint8)])])
        for i in np.flatnonzero(bad[k:] == bad[:-k]):
            w = t[i:i + k]
            if w in seen:
                continue
            seen.add(w)
            out.add(min(int(w.translate(_DIGIT), 4), int(w.translate(_COMP)[::-1].translate(_DIGIT), 4)))
    return sorted(out)


class World:
    """clusters + counts + the oracle's scored results for one (k, -prob or not)"""


@functools.lru_cache(maxsize=None)
def world(k, use_prob, n_random):
    w = World()
    w.k, w.use_prob = k, use_prob
    w.clusters = hand_clusters(k) + random_clusters(k, 77 * k + 5, n_random)
    w.unscored = [traverse_oracle(c) for c in w.clusters]
    kmers = canonical_kmers(k, [p for x in w.unscored for p in x["paths"]])
    r = np.random.default_rng(31 * k + (1 if use_prob else 0))
    rnames, anames = list(READ_PALETTE), list(ASM_PALETTE)
    w.read_class = r.integers(0, len(rnames), size=len(kmers))
    w.asm_class = r.integers(0, len(anames), size=len(kmers))
    rv = np.array([READ_PALETTE[rnames[i]] for i in w.read_class], dtype=np.uint64)
    av = np.array([ASM_PALETTE[anames[i]] for i in w.asm_class], dtype=np.uint64)
    w.read_classes = {rnames[i] for i in set(w.read_class.tolist())}
    w.asm_classes = {anames[i] for i in set(w.asm_class.tolist())}
    w.R = {x: int(v) for x, v in zip(kmers, rv) if v}
    w.A = {x: int(v) for x, v in zip(kmers, av) if v}
    w.probK, w.probP = (PROB_K, PROB_P) if use_prob else ([], [])
    w.params = po.Params(k, PEAK, w.probK or None, w.probP or None)
    if k <= 31:
        rk, ak = sorted(w.R), sorted(w.A)
        Rl = po.Lookup(k, np.array(rk, dtype=np.uint64), np.array([w.R[x] for x in rk], dtype=np.uint32))
        Al = po.Lookup(k, np.array(ak, dtype=np.uint64), np.array([w.A[x] for x in ak], dtype=np.uint32))
        w.scored = [po.cluster_paths(w.params, Rl, Al, c.win, c.variants, need_dk=True) for c in w.clusters]
    else:                                                    # the callback form: the k-mer's text, arbitrary-precision k-mers (oracle/plain.py)
        memo = {}

        def getk(text):
            v = memo.get(text)
            if v is None:
                f, rc = int(text.translate(_DIGIT), 4), int(text.translate(_COMP)[::-1].translate(_DIGIT), 4)
                readV = (w.R.get(f, 0) + (w.R.get(rc, 0))) & 0xffffffff if f != rc else (2 * w.R.get(f, 0)) & 0xffffffff
                asmV = (w.A.get(f, 0) + (w.A.get(rc, 0))) & 0xffffffff if f != rc else (2 * w.A.get(f, 0)) & 0xffffffff
                v = memo[text] = plain.getK(PEAK, w.probK, w.probP, readV, asmV)
            return v

        fn = po.getk_text_fn(getk)
        w.scored = [po.cluster_paths(w.params, None, None, c.win, c.variants, need_dk=True, cb=fn) for c in w.clusters]
    for a, b in zip(w.unscored, w.scored):
        assert a["paths"] == b["paths"] and a["status"] == b["status"]
    return w


def build_index(m, w):
    """the full index over the world's counts (Index.add_read / add_asm directly)"""
    def to_rows(ints):                                       # k > 31 at the C ABI: rows [low 64 bits, high bits]
        return np.array([[x & 0xffffffffffffffff, x >> 64] for x in ints], dtype=np.uint64).reshape(len(ints), 2)

    ix = m.Index(w.k, len(w.R) + len(w.A) + 16)
    rk, ak = sorted(w.R), sorted(w.A)
    conv = to_rows if w.k > 31 else (lambda x: np.array(x, dtype=np.uint64))
    ix.add_read(conv(rk), np.array([w.R[x] for x in rk], dtype=np.uint32))
    ix.add_asm(conv(ak), np.array([w.A[x] for x in ak], dtype=np.uint32))
    return ix
