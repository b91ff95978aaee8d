"""What `-track` must produce, derived from the per-position values of the oracle's -dump (oracle.pyoracle.process_dump;
oracle.plain.py_dump for 32 <= k <= 64, where the C oracle's 64-bit k-mers end): the window records as Python integers
and floats, and the text of the three files.  Every count is an integer, the sum of K* is a Python int in units of
2^-52 -- `int(kstar * 2**52)`, exact because a finite K* is +-(q - 1) with q >= 1 a double, a multiple of
ulp(q) >= 2^-52 -- and min / max are the doubles themselves, so the comparison with the device's records is `==`."""
import numpy as np

FIELDS = ("n_kmers", "n_missing", "n_scored", "n_pos", "n_neg", "n_nonfinite", "sum_readK", "sum_asmK", "sum_kstar",
          "min_kstar", "max_kstar")


def valid_starts(contig, k):
    """mask of the positions where a valid k-mer starts (all k bases ACGT, either case: kmerIterator)"""
    b = np.frombuffer(contig, dtype=np.uint8) & 0xDF
    ok = (b == 65) | (b == 67) | (b == 71) | (b == 84)
    n = len(b)
    out = np.zeros(n, dtype=bool)
    if n >= k:
        c = np.concatenate([[0], np.cumsum(ok)])
        out[:n - k + 1] = (c[k:] - c[:n - k + 1]) == k
    return out


def per_position_c(po, p, R, A, contig):
    """(valid, readK, asmK, K*) per start position from the C oracle's processDump"""
    rk, ak, km, kasm, kmiss = po.process_dump(p, R, A, contig)
    n = len(contig)
    valid = valid_starts(contig, p.k)
    assert int(valid.sum()) == kasm and int((valid & (rk[:n] == 0)).sum()) == kmiss
    assert not rk[:n][~valid].any() and not ak[:n][~valid].any() and not km[:n][~valid].any()
    return valid, rk[:n], ak[:n], km[:n]


def per_position_plain(plain, k, peak, probK, probP, contig, R, A):
    """the same from the plain-Python restatement (contig: str; R, A: dicts of canonical k-mer counts)"""
    n = len(contig)
    valid = np.zeros(n, dtype=bool)
    rk, ak, km = np.zeros(n), np.zeros(n), np.zeros(n)
    for i, w in plain.valid_kmers(contig, k):
        readV, asmV = plain.values(k, w, R, A)
        a, b, _ = plain.getK(peak, probK, probP, readV, asmV)
        valid[i] = True
        rk[i], ak[i] = a, b
        km[i] = plain.kmetric(a, b) if (a == 0 or b != 0) else float("inf")       # readK / 0 (getKmetric in C: inf)
    return valid, rk, ak, km


def reduce_windows(pp, W):
    """pp: per contig (valid, readK, asmK, K*) -> the list of window records (dicts), contig by contig"""
    out = []
    for valid, rk, ak, km in pp:
        n = len(valid)
        if n == 0:
            continue
        starts = np.arange(0, n, W, dtype=np.int64)
        missing = valid & (rk == 0)
        nonfin = valid & (rk != 0) & ~np.isfinite(km)
        assert np.array_equal(nonfin, valid & (rk != 0) & (ak == 0))               # the only way K* is not finite
        scored = valid & ~missing & ~nonfin
        red = lambda a: np.add.reduceat(a.astype(np.uint64), starts)
        rki = np.where(scored, rk, 0)
        aki = np.where(scored, ak, 0)
        assert np.array_equal(rki, np.floor(rki)) and np.array_equal(aki, np.floor(aki))
        cols = {"n_kmers": red(valid), "n_missing": red(missing), "n_scored": red(scored), "n_pos": red(scored & (km > 0)),
                "n_neg": red(scored & (km < 0)), "n_nonfinite": red(nonfin), "sum_readK": red(rki), "sum_asmK": red(aki)}
        mn = np.minimum.reduceat(np.where(scored, km, np.inf), starts)
        mx = np.maximum.reduceat(np.where(scored, km, -np.inf), starts)
        # the exact sum: Python integers, units of 2^-52
        pref = [0]
        for s, x in zip(scored.tolist(), km.tolist()):
            if s:
                y = x * 2.0 ** 52
                assert y.is_integer(), x
                pref.append(pref[-1] + int(y))
            else:
                pref.append(pref[-1])
        for i, s in enumerate(starts.tolist()):
            e = min(s + W, n)
            r = {f: int(cols[f][i]) for f in cols}
            r["sum_kstar"] = pref[e] - pref[s]
            r["min_kstar"], r["max_kstar"] = float(mn[i]), float(mx[i])
            out.append(r)
    return out


def device_records(w):
    """the structured array of Evaluator.track as the same dicts"""
    out = []
    for x in w:
        r = {f: int(x[f]) for f in FIELDS[:8]}
        r["sum_kstar"] = (int(x["sum_kstar_hi"]) << 64) + int(x["sum_kstar_lo"])
        r["min_kstar"], r["max_kstar"] = float(x["min_kstar"]), float(x["max_kstar"])
        out.append(r)
    return out


def mean_kstar(r):
    """nearest double to the exact sum * 2^-52 (int / int is correctly rounded), over the number of scored k-mers"""
    return (r["sum_kstar"] / 2 ** 52) / float(r["n_scored"])


def format_files(recs, names, lens, W):
    """the text of <out>.track.tsv, <out>.kstar.bedgraph and <out>.missing.bedgraph"""
    tsv = ["#name\tstart\tend\tn_kmers\tn_missing\tn_scored\tn_pos\tn_neg\tsum_readK\tsum_asmK\tmean_kstar\tmin_kstar\tmax_kstar\n"]
    bg = ['track type=bedGraph name="K*"\n']
    ms = ['track type=bedGraph name="missing"\n']
    i = 0
    for name, n in zip(names, lens):
        for s in range(0, n, W):
            r = recs[i]
            i += 1
            e = min(s + W, n)
            if r["n_kmers"]:
                mean = mean_kstar(r) if r["n_scored"] else 0.0
                tsv.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\n" % (
                    name, s, e, r["n_kmers"], r["n_missing"], r["n_scored"], r["n_pos"], r["n_neg"], r["sum_readK"], r["sum_asmK"],
                    mean, r["min_kstar"], r["max_kstar"]))
                ms.append("%s\t%d\t%d\t%.6f\n" % (name, s, e, r["n_missing"] / r["n_kmers"]))
            if r["n_scored"]:
                bg.append("%s\t%d\t%d\t%.6f\n" % (name, s, e, mean_kstar(r)))
    assert i == len(recs)
    return "".join(tsv), "".join(bg), "".join(ms)
