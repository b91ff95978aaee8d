"""What `-phase` must produce (include/merfin_amd.h, at mfx_phase_block), as a plain sequential walk over the markers of every contig
in Python integers: markers -> runs -> short / long -> blocks.  Nothing here is shaped like the device's steps (no words, no scans):
it is the rule as the documents state it.  Every field is an integer, so the comparison with the device's records is `==`.  Also the
two haplotype planes of hand-made markers and the three output texts."""
import numpy as np

FIELDS = ("contig", "hap", "start", "end", "n_hap", "n_switch", "n_switch_runs")
TILE = 4096
BED_HEADER = "#chrom\tstart\tend\thap\tn_hap\tn_switch\tn_switch_runs\n"
COUNT_HEADER = "#chrom\tA\tB\tshared\tkmers\n"
STATS_HEADER = "#set\tblocks\tsum\tmin\tmean\tmax\tN50\tmarkers\tswitch_markers\tswitch_rate\n"


def runs_of(markers):
    """markers: [(position, hap)] ascending -> runs [hap, first, last, n]: maximal stretches of consecutive markers of one haplotype"""
    runs = []
    for p, h in markers:
        if runs and runs[-1][0] == h:
            runs[-1][2] = p
            runs[-1][3] += 1
        else:
            runs.append([h, p, p, 1])
    return runs


def is_short(run, k, S, R):
    _, first, last, n = run
    return n <= S and last - first + k <= R


def blocks_of_contig(contig, markers, k, S, R):
    """the blocks of one contig as dicts"""
    blocks = []                                               # each: list of runs
    last_long = None                                          # haplotype of the nearest earlier long run
    for run in runs_of(markers):
        long_ = not is_short(run, k, S, R)
        if not blocks or (long_ and last_long is not None and last_long != run[0]):
            blocks.append([])
        blocks[-1].append(run)
        if long_:
            last_long = run[0]
    out = []
    for runs in blocks:
        longs = {r[0] for r in runs if not is_short(r, k, S, R)}
        assert len(longs) <= 1
        n = [sum(r[3] for r in runs if r[0] == h) for h in (0, 1)]
        if longs:
            hap = longs.pop()
        else:
            assert len(blocks) == 1
            hap = 1 if n[1] > n[0] else 0
        out.append({"contig": contig, "hap": hap, "start": runs[0][1], "end": runs[-1][2] + 1, "n_hap": n[hap], "n_switch": n[1 - hap],
                    "n_switch_runs": sum(1 for r in runs if r[0] != hap)})
    return out


def blocks(markers_per_contig, k, S, R):
    """markers_per_contig: per contig [(position, hap)] ascending -> the expected records, ordered by contig, start"""
    out = []
    for c, mk in enumerate(markers_per_contig):
        out += blocks_of_contig(c, mk, k, S, R)
    return out


def markers_of_masks(a, b):
    """two boolean arrays over a contig's positions (in A and not in B; in B and not in A) -> [(position, hap)]"""
    assert not (a & b).any()
    pos = np.flatnonzero(a | b)
    return [(int(p), int(b[p])) for p in pos]


def device_records(arr):
    """the structured array of Evaluator.phase / phase_from_planes_host as the same dicts"""
    return [{f: int(x[f]) for f in FIELDS} for x in arr]


def planes_of(markers_per_contig, lens):
    """the two haplotype planes the device makes: uint64 [2][ntiles * 64], bit b of word w of a tile = position 64 w + b of the tile"""
    ntiles = sum((n + TILE - 1) // TILE for n in lens)
    planes = np.zeros((2, ntiles * 64), dtype=np.uint64)
    t0 = 0
    for mk, n in zip(markers_per_contig, lens):
        nt = (n + TILE - 1) // TILE
        for p, h in mk:
            assert 0 <= p < n
            planes[h, t0 * 64 + p // 64] |= np.uint64(1) << np.uint64(p % 64)
        t0 += nt
    return planes


def format_bed(recs, names, k):
    """<out>.phased_block.bed: columns 2 and 3 are the base span [start, end - 1 + k)"""
    out = [BED_HEADER]
    for r in (recs if isinstance(recs, list) else device_records(recs)):
        out.append("%s\t%d\t%d\t%s\t%d\t%d\t%d\n" % (names[r["contig"]], r["start"], r["end"] - 1 + k, "AB"[r["hap"]], r["n_hap"], r["n_switch"],
                                                   r["n_switch_runs"]))
    return "".join(out)


def format_counts(contig_counts, names):
    """<out>.hapmers.count: contig_counts[c] = (valid k-mers, A markers, B markers, shared)"""
    out = [COUNT_HEADER]
    for name, (valid, a, b, shared) in zip(names, contig_counts):
        out.append("%s\t%d\t%d\t%d\t%d\n" % (name, int(a), int(b), int(shared), int(valid)))
    return "".join(out)


def _stats_line(name, recs, k):
    spans = sorted((r["end"] - 1 + k - r["start"] for r in recs), reverse=True)
    total = sum(spans)
    n50 = 0
    for L in sorted(set(spans)):                              # the largest L such that blocks of span >= L hold at least half the sum
        if 2 * sum(s for s in spans if s >= L) >= total:
            n50 = L
    markers = sum(r["n_hap"] + r["n_switch"] for r in recs)
    switches = sum(r["n_switch"] for r in recs)
    n = len(spans)
    return "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\n" % (name, n, total, spans[-1] if n else 0, total // n if n else 0, spans[0] if n else 0, n50, markers,
                                                           switches, switches / markers if markers else 0.0)


def format_stats(recs, k, S, R):
    """<out>.phased_block.stats: for A, B and all"""
    recs = recs if isinstance(recs, list) else device_records(recs)
    return ("#switches\t%d\trange\t%d\tk\t%d\n" % (S, R, k) + STATS_HEADER + _stats_line("A", [r for r in recs if r["hap"] == 0], k) +
            _stats_line("B", [r for r in recs if r["hap"] == 1], k) + _stats_line("all", recs, k))
