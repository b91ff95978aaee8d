"""What `-bin` must produce (include/merfin_amd.h, at mfx_bin_record), as a plain sequential walk over every read in Python integers:
the kmerIterator rules (k valid bases in a row, either case; anything else starts over), the canonical k-mer -- or, for a set that is
not canonical, the forward and the reverse-complement k-mer both looked up -- and membership in two Python sets.  Nothing here is
shaped like the device's steps (no batches, no pieces, no tiles).  The class rule is written with Python integers, and the texts of the
command line are formatted here.  Every field is an integer, so the comparison with the device's records is `==`."""

CODE = {}
for _c, _v in (("A", 0), ("C", 1), ("T", 2), ("G", 3)):      # (c >> 1) & 3 of the letter, as the library packs it
    CODE[ord(_c)] = _v
    CODE[ord(_c.lower())] = _v

TSV_HEADER = "#read\tlength\tkmers\tA\tB\tshared\tclass\n"
STATS_HEADER = "#class\treads\tbases\tkmers\tA\tB\tshared\n"
CLASS_NAMES = "ABU"


def read_counts(read, k, A, B, canonical=True):
    """(valid k-mers, in A only, in B only, in both) of one read; A, B: Python sets of integers"""
    mask = (1 << (2 * k)) - 1
    top = 2 * (k - 1)
    f = r = run = 0
    n = na = nb = ns = 0
    for ch in read:
        c = CODE.get(ch)
        if c is None:
            run = 0
            continue
        f = ((f << 2) | c) & mask
        r = (r >> 2) | ((c ^ 2) << top)
        run += 1
        if run < k:
            continue
        if canonical:
            x = f if f < r else r
            ina, inb = x in A, x in B
        else:
            ina, inb = (f in A) or (r in A), (f in B) or (r in B)
        n += 1
        if ina and inb:
            ns += 1
        elif ina:
            na += 1
        elif inb:
            nb += 1
    return (n, na, nb, ns)


def counts(reads, k, A, B, canonical=True):
    """one row per read, in input order"""
    A, B = set(int(x) for x in A), set(int(x) for x in B)
    return [read_counts(rd if isinstance(rd, (bytes, bytearray)) else rd.encode(), k, A, B, canonical) for rd in reads]


def classify(a, b, norm_a, norm_b, ratio_milli=1000, min_hits=1):
    """0 A, 1 B, 2 unknown"""
    assert ratio_milli >= 1000
    NA, NB = norm_a or 1, norm_b or 1
    if a + b >= min_hits and a * NB * 1000 > b * NA * ratio_milli:
        return 0
    if a + b >= min_hits and b * NA * 1000 > a * NB * ratio_milli:
        return 1
    return 2


def classes(rows, norm_a, norm_b, ratio_milli=1000, min_hits=1):
    return [classify(r[1], r[2], norm_a, norm_b, ratio_milli, min_hits) for r in rows]


def format_tsv(names, lens, rows, cls):
    out = [TSV_HEADER]
    for name, n, r, c in zip(names, lens, rows, cls):
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (name, n, r[0], r[1], r[2], r[3], CLASS_NAMES[c]))
    return "".join(out)


def format_stats(lens, rows, cls, k, norm_a, norm_b, ratio_milli=1000, min_hits=1):
    out = ["#ratio\t%d.%03d\tminhits\t%d\tk\t%d\tnorm_A\t%d\tnorm_B\t%d\n" % (ratio_milli // 1000, ratio_milli % 1000, min_hits, k, norm_a, norm_b), STATS_HEADER]
    for name, want in (("A", (0,)), ("B", (1,)), ("U", (2,)), ("all", (0, 1, 2))):
        sel = [i for i, c in enumerate(cls) if c in want]
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, len(sel), sum(lens[i] for i in sel), sum(rows[i][0] for i in sel), sum(rows[i][1] for i in sel),
                                                   sum(rows[i][2] for i in sel), sum(rows[i][3] for i in sel)))
    return "".join(out)


def format_fasta(names, reads, cls, want):
    """the records of class `want`, name and bases as read, in input order"""
    return "".join(">%s\n%s\n" % (n, r.decode() if isinstance(r, (bytes, bytearray)) else r) for n, r, c in zip(names, reads, cls) if c == want)
