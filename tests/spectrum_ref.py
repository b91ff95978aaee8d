"""Reference model of the copy-number spectrum (include/merfin_amd.h: mfx_spectrum_run, mfx_spectrum_peak,
mfx_spectrum_write), written independently of the C++ and of any GPU index: the image from the (kmers, counts) tables the
synthetic worlds return, joined with numpy; the peak rule restated with fractions.Fraction; the report as a string."""
from fractions import Fraction

import numpy as np


def _keys(k):
    """k-mers as one comparable array: uint64, or (n, 2) rows [low 64 bits, high bits] (k > 31) as a structured array"""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    if k.ndim == 2:
        s = np.empty(len(k), dtype=[("hi", np.uint64), ("lo", np.uint64)])
        s["hi"], s["lo"] = k[:, 1], k[:, 0]
        return s
    return k


def join(read, asm):
    """(read count, assembly count) of every k-mer of either table, uint64 each; the k-mers of a table are distinct"""
    rk, ak = _keys(read[0]), _keys(asm[0])
    if len(rk) + len(ak) == 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    both = np.concatenate([rk, ak]) if len(rk) and len(ak) else (rk if len(rk) else ak)
    u, inv = np.unique(both, return_inverse=True)
    r = np.zeros(len(u), dtype=np.uint64)
    a = np.zeros(len(u), dtype=np.uint64)
    r[inv[:len(rk)]] = np.asarray(read[1], dtype=np.uint64)
    a[inv[len(rk):]] = np.asarray(asm[1], dtype=np.uint64)
    return r, a


def image_of_pairs(r, a, copies, max_mult, minV=0, maxV=2 ** 64 - 1, seq_only=False):
    r = np.asarray(r, dtype=np.uint64).copy()
    a = np.asarray(a, dtype=np.uint64)
    if seq_only:                                      # the table holds the assembly's k-mers only
        r, a = r[a > 0], a[a > 0]
    r[(r < np.uint64(minV)) | (r > np.uint64(min(maxV, 2 ** 64 - 1)))] = 0        # -min / -max: outside the filter the read count is 0
    keep = (r != 0) | (a != 0)
    r, a = r[keep], a[keep]
    row = np.where(a <= copies, a, copies + 1).astype(np.int64)
    col = np.minimum(r, np.uint64(max_mult)).astype(np.int64)
    img = np.zeros((copies + 2, max_mult + 1), dtype=np.uint64)
    np.add.at(img, (row, col), np.uint64(1))
    return img


def image(read, asm, copies, max_mult, minV=0, maxV=2 ** 64 - 1, seq_only=False):
    r, a = join(read, asm)
    return image_of_pairs(r, a, copies, max_mult, minV, maxV, seq_only)


def peak(row):
    """the rule of mfx_spectrum_peak on a row of max_mult + 1 cells: (valley, main peak, haploid peak, row[haploid peak]) or None"""
    row = [int(x) for x in row]
    M = len(row) - 1
    assert M >= 4
    pre = [0]
    for x in row:
        pre.append(pre[-1] + x)

    def mean(m):
        lo, hi = max(1, m - 2), min(M - 1, m + 2)
        return Fraction(pre[hi + 1] - pre[lo], hi - lo + 1)

    # (beyond E -- three past the last occupied cell that takes part -- every mean is 0: such m cannot be the first point of a
    # positive maximum, and where the maximum is 0 there is no peak; they are not evaluated one by one)
    E = min(M, max([j for j in range(1, M) if row[j]], default=0) + 4)
    A = [None] + [mean(m) for m in range(1, E)] + [Fraction(0)] * (M - E)
    v = next((m for m in range(1, min(M - 1, E)) if A[m] <= A[m + 1]), None)
    if v is None:
        return None
    top = max(A[v + 1:max(E, v + 2)])
    if top == 0:
        return None
    p = next(m for m in range(v + 1, M) if A[m] == top)
    hap = p
    lo, hi = max(v + 1, -((-2 * p) // 5)), (3 * p) // 5           # ceil(0.4 p), floor(0.6 p)
    if lo <= hi:
        best = max(A[lo:hi + 1])
        h = next(m for m in range(lo, hi + 1) if A[m] == best)
        near = range(max(1, h - 2), min(M - 1, h + 2) + 1)
        if 10 * A[h] >= A[p] and all(A[h] >= A[j] for j in near):
            hap = h
    return v, p, hap, row[hap]


def text(img, with_read_only=True):
    img = np.asarray(img)
    copies, max_mult = img.shape[0] - 2, img.shape[1] - 1
    out = ["Copies\tkmer_multiplicity\tCount\n"]
    for r in range(0 if with_read_only else 1, copies + 2):
        label = "read-only" if r == 0 else (str(r) if r <= copies else ">%d" % copies)
        for m in range(max_mult + 1):
            if int(img[r, m]):
                out.append("%s\t%d\t%d\n" % (label, m, int(img[r, m])))
    return "".join(out)
