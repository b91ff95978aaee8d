"""What `-regions` must produce, derived from the per-position values of the oracle's -dump (tests/track_ref.py: per_position_c;
per_position_plain for 32 <= k <= 64): class arrays, elementary runs by np.diff, the joining over gaps, the filter, the sums --
numpy and Python integers only -- and the BED text.  Every field is an integer or the double of one position, so the comparison
with the device's records is `==`."""
import numpy as np

CLASSES = ("missing", "collapsed", "expanded")
FIELDS = ("contig", "cls", "start", "end", "n_kmers", "sum_readK", "sum_asmK", "ext_kstar")
TILE = 4096


def class_masks(valid, rk, ak, km, t):
    """the three class masks of one contig (include/merfin_amd.h, at mfx_region)"""
    missing = valid & (rk == 0)
    scored = valid & (rk != 0) & (ak != 0)
    with np.errstate(invalid="ignore"):
        collapsed = scored & (km >= t)
        expanded = scored & (km <= -t)
    assert not (missing & collapsed).any() and not (missing & expanded).any() and not (collapsed & expanded).any()
    return missing, collapsed, expanded


def runs(mask):
    """maximal stretches of True as (starts, ends), ends exclusive"""
    d = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)


REF_DTYPE = np.dtype([("contig", "<u4"), ("cls", "<u4"), ("start", "<u8"), ("end", "<u8"), ("n_kmers", "<u8"), ("sum_readK", "<u8"),
                      ("sum_asmK", "<u8"), ("ext_kstar", "<f8")])


def join_runs(starts, ends, gap):
    """runs in order -> (index of each region's first run, region starts, region ends, flagged k-mers): a run joins the region in
    front of it while at most `gap` positions lie between that region's last flagged position and the run's first"""
    if len(starts) == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z
    head = np.concatenate([[True], starts[1:] - ends[:-1] > gap])
    first = np.flatnonzero(head)
    last = np.concatenate([first[1:] - 1, [len(starts) - 1]])
    return first, starts[first], ends[last], np.add.reduceat(ends - starts, first)


def regions_array(masks, gap, min_kmers, values=None):
    """masks: per contig the three class masks; values: per contig (rk, ak, km) or None (sums 0).  The records as a structured
    array in the records' order: contig, start, class."""
    parts = []
    for c, m3 in enumerate(masks):
        mine = []
        for cls, mask in enumerate(m3):
            rs, re = runs(mask)
            first, s, e, n = join_runs(rs, re, gap)
            r = np.zeros(len(s), dtype=REF_DTYPE)
            r["contig"], r["cls"], r["start"], r["end"], r["n_kmers"] = c, cls, s, e, n
            if values is not None and len(s):
                rk, ak, km = values[c]
                a, b = np.where(mask, rk, 0), np.where(mask, ak, 0)
                assert np.array_equal(a, np.floor(a)) and np.array_equal(b, np.floor(b))
                # every flagged position from a region's start up to the next region's start is the region's own
                r["sum_readK"] = np.add.reduceat(a.astype(np.uint64), s)
                r["sum_asmK"] = np.add.reduceat(b.astype(np.uint64), s)
                assert np.array_equal(np.add.reduceat(mask.astype(np.uint64), s), r["n_kmers"])
                if cls == 1:
                    r["ext_kstar"] = np.maximum.reduceat(np.where(mask, km, -np.inf), s)
                elif cls == 2:
                    r["ext_kstar"] = np.minimum.reduceat(np.where(mask, km, np.inf), s)
            mine.append(r[r["n_kmers"] >= min_kmers])
        mine = np.concatenate(mine)
        parts.append(mine[np.lexsort((mine["cls"], mine["start"]))])
    return np.concatenate(parts) if parts else np.zeros(0, dtype=REF_DTYPE)


def regions_from_masks(masks, gap, min_kmers, values=None):
    """the same as dicts"""
    return device_records(regions_array(masks, gap, min_kmers, values))


def same_records(got, want):
    """every field of every record, compared with ==; returns the first difference (None: equal)"""
    if len(got) != len(want):
        return ("count", len(got), len(want))
    for f in FIELDS:
        if not np.array_equal(got[f], want[f]):
            i = int(np.flatnonzero(got[f] != want[f])[0])
            return (f, i, got[i], want[i])
    return None


def masks_of(pp, t):
    return [class_masks(valid, rk, ak, km, t) for valid, rk, ak, km in pp]


def regions(pp, t, gap, min_kmers, masks=None):
    """pp: per contig (valid, readK, asmK, K*) -> the expected records (a structured array with the fields of mfx_region)"""
    return regions_array(masks if masks is not None else masks_of(pp, t), gap, min_kmers, [(rk, ak, km) for _, rk, ak, km in pp])


def flagged_tiles(masks):
    """tiles (4096 start positions of one contig) that hold a flagged position"""
    n = 0
    for m3 in masks:
        any3 = m3[0] | m3[1] | m3[2]
        for s in range(0, len(any3), TILE):
            n += bool(any3[s:s + TILE].any())
    return n


def device_records(a):
    """the structured array of Evaluator.regions as the same dicts"""
    return [{"contig": int(x["contig"]), "cls": int(x["cls"]), "start": int(x["start"]), "end": int(x["end"]), "n_kmers": int(x["n_kmers"]),
             "sum_readK": int(x["sum_readK"]), "sum_asmK": int(x["sum_asmK"]), "ext_kstar": float(x["ext_kstar"])} for x in a]


HEADER = "#chrom\tstart\tend\tclass\tn_kmers\tmean_readK\tmean_asmK\text_kstar\n"


def format_bed(recs, names, k):
    """the text of <out>.regions.bed: columns 2 and 3 are the base span [start, end - 1 + k)"""
    out = [HEADER]
    for r in (recs if isinstance(recs, list) else device_records(recs)):
        out.append("%s\t%d\t%d\t%s\t%d\t%.2f\t%.2f\t%.2f\n" % (names[r["contig"]], r["start"], r["end"] - 1 + k, CLASSES[r["cls"]], r["n_kmers"],
                                                            float(r["sum_readK"]) / float(r["n_kmers"]), float(r["sum_asmK"]) / float(r["n_kmers"]),
                                                            r["ext_kstar"]))
    return "".join(out)


def planes_of(masks, lens):
    """the class planes the device makes: uint64 [3][ntiles * 64], bit b of word w of a tile = position 64 w + b of the tile"""
    ntiles = sum((n + TILE - 1) // TILE for n in lens)
    planes = np.zeros((3, ntiles * 64), dtype=np.uint64)
    t0 = 0
    for m3, n in zip(masks, lens):
        nt = (n + TILE - 1) // TILE
        for cls in range(3):
            bits = np.zeros(nt * TILE, dtype=np.uint8)
            bits[:n] = m3[cls]
            words = np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)
            planes[cls, t0 * 64:(t0 + nt) * 64] = words
        t0 += nt
    return planes
