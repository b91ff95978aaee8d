"""A plain numpy reference of what mfx_db_diploid computes (include/merfin_amd.h), from np.union1d and searchsorted over the three arrays.
It shares no code with the library: the four results are written here from their definitions.

For every distinct k-mer of the union: r the raw read count (0: absent), rf = r where lo <= r <= hi and else 0, c1 / c2 the counts in hap1 /
hap2, cb = min(c1 + c2, 2^32 - 1)."""
import numpy as np

TOP = 2**32 - 1
NAMES = ("hap1", "hap2", "both")


def spread(reads, hap1, hap2):
    """(k-mers of the union ascending, r, c1, c2) as uint64 arrays"""
    u = np.union1d(np.union1d(np.asarray(reads[0], dtype=np.uint64), np.asarray(hap1[0], dtype=np.uint64)), np.asarray(hap2[0], dtype=np.uint64))
    cols = []
    for keys, vals in (reads, hap1, hap2):
        c = np.zeros(len(u), dtype=np.uint64)
        c[np.searchsorted(u, np.asarray(keys, dtype=np.uint64))] = np.asarray(vals, dtype=np.uint64)
        cols.append(c)
    return (u,) + tuple(cols)


def read_k(peak, prob, r):
    """merfin's readK of read counts r > 0 (merfin-globals.C:80-97) as float64; prob: (probK, probP) rows for the counts 1 .. len, or None"""
    r = np.asarray(r, dtype=np.uint64)
    rd = r.astype(np.float64)
    q = rd / np.float64(peak)
    out = np.where(rd < peak, 1.0, np.floor(q + 0.5))              # round half away from zero (q > 0)
    if prob is not None and len(prob[0]):
        pk = np.asarray(prob[0], dtype=np.float64)
        inside = r <= np.uint64(len(pk))
        out = np.where(inside, pk[np.minimum(r, np.uint64(len(pk))).astype(np.int64) - 1], out)
    return out


def diploid(reads, hap1, hap2, k, copies=4, max_mult=10000, lo=0, hi=TOP, peak=None, prob=None):
    """the dict m.db_diploid returns, without the times and the windows"""
    u, r, c1, c2 = spread(reads, hap1, hap2)
    rf = np.where((r < np.uint64(lo)) | (r > np.uint64(hi)), np.uint64(0), r)
    cb = np.minimum(c1 + c2, np.uint64(TOP))
    col = np.minimum(rf, np.uint64(max_mult)).astype(np.int64)
    entry = (rf > 0) | (cb > 0)
    cls = np.where(c1 > 0, np.where(c2 > 0, 3, 1), np.where(c2 > 0, 2, 0))
    asm_img = np.zeros((4, max_mult + 1), dtype=np.uint64)
    np.add.at(asm_img, (cls[entry], col[entry]), np.uint64(1))
    cn_img = np.zeros((copies + 2, max_mult + 1), dtype=np.uint64)
    np.add.at(cn_img, (np.minimum(cb, np.uint64(copies + 1)).astype(np.int64)[entry], col[entry]), np.uint64(1))
    stats = {}
    for name, cx in zip(NAMES, (c1, c2, cb)):
        held, only = cx > 0, (cx > 0) & (r == 0)
        stats[name] = {"distinct": int(held.sum()), "total": int(cx.sum(dtype=np.uint64)), "only_distinct": int(only.sum()),
                       "only_total": int(cx[only].sum(dtype=np.uint64)), "found": int((held & (rf > 0)).sum())}
    stats.update(solid=int((rf > 0).sum()), n_read=int((r > 0).sum()), n_hap1=int((c1 > 0).sum()), n_hap2=int((c2 > 0).sum()),
                 n_shared=int(((c1 > 0) & (c2 > 0)).sum()))
    out = {"asm_img": asm_img, "cn_img": cn_img, "n_entries": int(entry.sum()), "stats": stats, "kmers": (u, r, c1, c2)}
    if peak is not None:
        piece = ((u >> np.uint64(max(2 * k - 6, 0))) & np.uint64(63)).astype(np.int64)
        have = r > 0
        rk = np.zeros(len(u), dtype=np.float64)
        rk[have] = read_k(peak, prob, r[have])
        total = np.zeros(64)
        np.add.at(total, piece[have], rk[have])
        und = np.zeros((3, 64))
        for i, cx in enumerate((c1, c2, cb)):
            d = rk - cx.astype(np.float64)
            sel = have & (d > 0)
            np.add.at(und[i], piece[sel], d[sel])
        out["total"], out["undrcpy"] = total, und
    return out


def same(got, want, times=False):
    """every field of two result dicts `==`; returns the first field that differs, or None"""
    for key in ("asm_img", "cn_img"):
        if not np.array_equal(got[key], want[key]):
            return key
    if got["n_entries"] != want["n_entries"]:
        return "n_entries"
    for key, v in want["stats"].items():
        if key.startswith("t_") or key == "windows":
            continue
        if got["stats"][key] != v:
            return "stats." + key
    for key in ("total", "undrcpy"):
        if (key in want) != (key in got) or (key in want and not np.array_equal(got[key], want[key])):
            return key
    return None
