"""The numpy reference of mfx_db_trio (include/merfin_amd.h; the rule: csrc/mfx_trio.h) and the worlds its tests share.  The reference takes
the union of the three key arrays, looks every count up with np.searchsorted and applies the rule as the issue states it in integers:
    A: cm >= tm and cp == 0 and (no child or cc >= tc), count min(cm, cc) or cm;  B: the same with the parents swapped
    image row 0: cp == 0 by cm; row 1: cm == 0 by cp; row 2: every child k-mer by cc; the last column takes max_mult and more"""
import numpy as np

from tests import stream_worlds as sw

SIZES = (0, 1, 4095, 4096, 4097, 20000)
EMPTY = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
COUNTERS = ("n_mat", "n_pat", "n_child", "n_both", "n_mat_only", "n_pat_only", "n_mat_only_cut", "n_pat_only_cut", "n_child_cut", "n_a", "n_b")


def _lookup(keys, vals, u):
    if len(keys) == 0:
        return np.zeros(len(u), dtype=np.uint64)
    at = np.minimum(np.searchsorted(keys, u), len(keys) - 1)
    return np.where(keys[at] == u, vals[at].astype(np.uint64), np.uint64(0)).astype(np.uint64)


def image(cm, cp, cc, max_mult):
    img = np.zeros((3, max_mult + 1), dtype=np.uint64)
    for r, c in enumerate((cm[(cp == 0) & (cm > 0)], cp[(cm == 0) & (cp > 0)], cc[cc > 0])):
        img[r] = np.bincount(np.minimum(c, np.uint64(max_mult)).astype(np.int64), minlength=max_mult + 1).astype(np.uint64)
    return img


def reference(mat, pat, child, tm, tp, tc=1, max_mult=10000):
    """((A k-mers, A counts), (B k-mers, B counts), image, counters) for (k-mers, counts) pairs; child None: no child"""
    has_child = child is not None
    ck, cv = child if has_child else EMPTY
    u = np.union1d(np.union1d(mat[0], pat[0]), ck).astype(np.uint64)
    cm, cp, cc = _lookup(mat[0], mat[1], u), _lookup(pat[0], pat[1], u), _lookup(ck, cv, u)
    child_ok = (cc >= tc) & (cc > 0) if has_child else np.ones(len(u), dtype=bool)
    in_a = (cm >= tm) & (cm > 0) & (cp == 0) & child_ok
    in_b = (cp >= tp) & (cp > 0) & (cm == 0) & child_ok
    assert not (in_a & in_b).any()
    va = (np.minimum(cm, cc) if has_child else cm)[in_a].astype(np.uint32)
    vb = (np.minimum(cp, cc) if has_child else cp)[in_b].astype(np.uint32)
    st = {"n_mat": len(mat[0]), "n_pat": len(pat[0]), "n_child": len(ck), "n_both": int(((cm > 0) & (cp > 0)).sum()),
          "n_mat_only": int(((cm > 0) & (cp == 0)).sum()), "n_pat_only": int(((cp > 0) & (cm == 0)).sum()),
          "n_mat_only_cut": int(((cm >= tm) & (cm > 0) & (cp == 0)).sum()), "n_pat_only_cut": int(((cp >= tp) & (cp > 0) & (cm == 0)).sum()),
          "n_child_cut": int(((cc >= tc) & (cc > 0)).sum()) if has_child else 0, "n_a": int(in_a.sum()), "n_b": int(in_b.sum())}
    return (u[in_a], va), (u[in_b], vb), image(cm, cp, cc, max_mult), st


def sets(k, sizes, seed, lo=1, hi=5, pool=30000):
    """databases of these sizes drawn from one pool of `pool` k-mers, so that every membership pattern occurs; counts lo .. hi - 1"""
    rng = np.random.default_rng(seed)
    pool = sw.random_keys(k, pool, seed)
    out = []
    for n in sizes:
        keys = np.sort(rng.choice(pool, size=n, replace=False)) if n else np.zeros(0, dtype=np.uint64)
        out.append((keys.astype(np.uint64), rng.integers(lo, hi, size=n).astype(np.uint32)))
    return out


def roles(case):
    """the sizes of (mat, pat, child) of case 0 .. 5: every size takes every role once"""
    return SIZES[case % 6], SIZES[(case + 2) % 6], SIZES[(case + 4) % 6]


def spectrum_counts(n, rng, peak=20):
    """counts whose histogram falls from 1 (sequencing errors) and rises again to a peak near `peak` (the genome's k-mers)"""
    err = np.minimum(rng.geometric(0.55, size=n), 6)
    real = np.maximum(rng.poisson(peak, size=n), 1)
    return np.where(rng.random(n) < 0.45, err, real).astype(np.uint32)


def auto_world(k=21, seed=7):
    """three databases of 20 000, 16 000 and 18 000 k-mers from one pool whose three histogram rows have a valley and a peak (near 20, 14 and 26)"""
    rng = np.random.default_rng(seed)
    pool = sw.random_keys(k, 30000, seed)
    out = []
    for n, peak in ((20000, 20), (16000, 14), (18000, 26)):
        keys = np.sort(rng.choice(pool, size=n, replace=False)).astype(np.uint64)
        out.append((keys, spectrum_counts(n, rng, peak)))
    return out


def chain(m, tmp, mat, pat, child, out, tm, tc):
    """set A by the existing calls: (mat - pat, count >= tm) intersected with (child, count >= tc); B: call with the parents swapped"""
    if child is None:
        m.db_merge_except([mat], [pat], out, min_count=tm)
        return out
    x, y = str(tmp / "chain_x.mfxk"), str(tmp / "chain_y.mfxk")
    m.db_merge_except([mat], [pat], x, min_count=tm)
    m.db_merge([child], y, min_count=tc)
    m.db_merge([x, y], out, op="intersect")
    return out
