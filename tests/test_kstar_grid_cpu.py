"""The K* grid (tests/kstar_grid.py) on the CPU: the C oracle against the exact plain-Python reference over every kept pair,
the coverage the grid promises (every tabulated over-copy entry, both sides of every threshold), and the host ABI's
getK / getKmetric over every kept pair.  The GPU file (tests/test_gpu_kstar_grid.py) then holds the device to the reference."""
import math
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import kstar_grid as kg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROB = os.path.join(ROOT, "tests", "golden", "example_lookup_table.txt")
NBINS_DEFAULT = 65536                    # Evaluator(..., nbins=0): include/merfin_amd.h, mfx_eval_create


def project_constants():
    """the table sizes of the code under test, read from its header: the one place the grid's parameters come from"""
    src = open(os.path.join(ROOT, "merfin_amd", "csrc", "mfx_internal.h")).read()

    def val(name):
        m = re.search(r"(?:constexpr\s+uint32_t\s+%s\s*=|#define\s+%s)\s+(\d+)" % (name, name), src)
        assert m, name
        return int(m.group(1))
    return dict(maxp=val("MFX_V_MAXP_LDS"), klut=val("MFX_KLUT"), nb_lds=val("MFX_NB_LDS"), field=val("MFX_CSAT"),
                block=val("MFX_BLOCK"), tile=val("MFX_TILE"))


PC = project_constants()
GRID = dict(maxp=PC["maxp"], klut=PC["klut"], nb_lds=PC["nb_lds"], field=PC["field"])
CONFIGS = {c[0]: c for c in kg.configs(PROB)}
_kept = {}


def kept_pairs(name):
    if name not in _kept:
        cfg = CONFIGS[name]
        cands = kg.candidates(cfg, nbins_list=(PC["nb_lds"], NBINS_DEFAULT), **GRID)
        _kept[name] = (cands, kg.keep(cands, cfg))
    return _kept[name]


def test_project_constants_are_the_ones_the_issue_was_written_for():
    assert (PC["maxp"], PC["klut"], PC["nb_lds"], PC["field"], PC["block"], PC["tile"]) == (1024, 32, 1024, 2047, 256, 4096)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_kept_pairs(name):
    cands, kept = kept_pairs(name)
    print("%s: %d candidates, %d kept" % (name, len(cands), len(kept)))
    if name == "peak2e-7":
        assert len(kept) >= 10000
        # readK(maxp - 1) does not fit a uint32: the device's readK table is off for this configuration
        assert kg.get_readk(PC["maxp"] - 1, *CONFIGS[name][1:])[0] >= 2.0 ** 32
    else:
        assert len(cands) > 36000 and len(cands) - len(kept) <= 0.02 * len(cands)


def _oracle(k, cfg, w):
    _, peak, probK, probP = cfg
    read, asm = kg.tables(w)
    p = po.Params(k, peak, probK or None, probP or None)
    g, ka, km, _ = po.hist_run(p, po.Lookup(k, *read), po.Lookup(k, *asm), w.contigs, threads=2, mode=0)
    return g, ka, km


@pytest.mark.parametrize("k", [21, 31, 22])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_oracle_equals_exact_reference(name, k):
    cfg = CONFIGS[name]
    _, kept = kept_pairs(name)
    w = kg.build_world(k, kept, set(kept), seed=1, palindromes=8 if k % 2 == 0 else 0)
    # the world's k-mers are the ones `meryl count` finds; every kept pair sits on one of them
    ck, cv = po.count_kmers(k, w.contigs)
    assert ck.tolist() == w.keys and len(w.keys) >= len(kept)
    assert set(w.pair_of.values()) == set(kept)
    if k % 2 == 0:
        assert w.n_pal >= 4
    ref = kg.reference(w, cfg)
    g, ka, km = _oracle(k, cfg, w)
    assert (g.kasm, g.kmissing) == (ref.kasm, ref.kmissing)
    np.testing.assert_array_equal(kg.trim(g.undr()), kg.dense(ref.undr))
    np.testing.assert_array_equal(kg.trim(g.over()), kg.dense(ref.over))
    assert ka.tolist() == ref.contig_kasm and km.tolist() == ref.contig_kmissing
    # a sequential fp64 sum of n_under non-negative terms: every partial sum is at most S (1 + small), each addition rounds by
    # at most half an ulp of it
    S = float(ref.S)
    err = abs(float(kg.Fraction(g.koverCpy) - ref.S))
    print("%s k=%d: n_under=%d S=%.6f oracle rel err %.2e (bound %.2e); F-S rel %.2e" % (
        name, k, ref.n_under, S, err / S, ref.n_under * 2.0 ** -53, abs(float(ref.F * kg.Fraction(1, 2 ** 52) - ref.S)) / S))
    assert ref.n_under > 1000 and err <= ref.n_under * 2.0 ** -53 * S
    if k == 21:
        _coverage(name, cfg, ref)


def _coverage(name, cfg, ref):
    maxp, klut, nb = PC["maxp"], PC["klut"], PC["nb_lds"]
    ev = {p: kg.evaluate(p[0], p[1], cfg) for p in ref.seen}
    far = {("u" if e[3] == "u" else "o", e[5]) for e in ev.values() if e[3] != "m" and e[5] >= nb}
    print("%s: %d distinct pairs at some position, %d distinct bins >= %d" % (name, len(ev), len(far), nb))
    assert len(far) > 300
    if name == "peak2e-7":                   # (no readK table on the device for this one: the rest is about the tables)
        return
    # every non-zero entry of the tabulated over-copy terms: readV < maxp, 1 <= readK < klut, readK < asmV < klut
    want = set()
    for rv in range(maxp):
        rk, _ = kg.get_readk(rv, *cfg[1:])
        if 1 <= rk < klut and rk == int(rk):
            want.update((rv, av) for av in range(1, klut) if av > rk)
    print("%s: %d tabulated over-copy entries" % (name, len(want)))
    assert want and want <= set(ev), len(want - set(ev))
    # both sides of every threshold, on the under and the over side wherever both can exist
    def sides(pred):
        return {e[3] for p, e in ev.items() if e[3] != "m" and pred(p, e)}
    for v in (maxp - 1, maxp):
        assert sides(lambda p, e: p[0] == v) == {"u", "o"}, ("readV", v)
    for v in (klut - 1, klut):
        assert sides(lambda p, e: e[0] == v) == {"u", "o"}, ("readK", v)
        assert sides(lambda p, e: p[1] == v) == {"u", "o"}, ("asmV", v)
    for b in (nb - 1, nb, NBINS_DEFAULT - 1, NBINS_DEFAULT):
        assert sides(lambda p, e: e[5] == b) == {"u", "o"}, ("bin", b)
    rows = len(cfg[2]) or 184
    for v in (rows, rows + 1):
        assert sides(lambda p, e: p[0] == v) == {"u", "o"}, ("prob row", v)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_host_abi_getK_over_every_kept_pair(name):
    import merfin_amd as m
    cfg = CONFIGS[name]
    _, peak, probK, probP = cfg
    kp = m.KParams(peak, probK or None, probP or None)
    _, kept = kept_pairs(name)
    for rv, av in kept:
        rk, ak, prob = kg.evaluate(rv, av, cfg)[:3]
        got = m.getK(kp, rv, av)
        assert got == (rk, ak, prob), (rv, av)
        want = kg.kmetric(rk, ak)
        assert m.getKmetric(rk, ak) == want or (math.isinf(want) and math.isinf(m.getKmetric(rk, ak))), (rv, av)
