"""One mfx_db_diploid call against the chain of the five existing calls it replaces.  Measured, not gated: no threshold is set on any of this.

The read database is that of tools/count_rate.py and tools/join_rate.py (a seeded i.i.d. genome of --mb Mb generated on the device, reads
of --len bases at --cov x, both strands, substitutions at --err per base, counted by the claiming counter).  hap1 is the genome counted as
one record; hap2 is a copy of it with a substitution every --every bases (1000: a PLACEHOLDER density, not a measured heterozygosity).  All
files are sorted flat files in tmpfs.  Before anything is timed one run of each leg is compared: the cn image and its entry count, and the
piece sums of hap1, hap2 and the merged database, must be equal.  Then, alternating, --reps times each, the whole call from the files with
MFX_DB_TIMING set (the kernels are waited for per window, the split is the library's own):
  (a) diploid: db_diploid(reads, hap1, hap2) with the piece sums;
  (b) chain:   db_merge([hap1, hap2]) -> M, db_join_completeness on hap1, hap2 and M, db_join_spectrum(reads, M).
The lines go to stdout and are appended to --profile (default profiles/diploid_rate.txt).

    python tools/diploid_rate.py [--mb 256] [--cov 30] [--len 150] [--err 0.005] [--k 21] [--every 1000] [--reps 5] [--out DIR] [--profile FILE]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.join_rate import _count_genome      # noqa: E402
from tools.merge_rate import _count_half       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--cov", type=float, default=30.0)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--every", type=int, default=1000, help="hap2: a substitution every this many bases of the genome (a placeholder density)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--peak", type=float, default=26.0)
    ap.add_argument("--out", default=None, help="directory of the databases (default: tmpfs)")
    ap.add_argument("--profile", default=os.path.join(ROOT, "profiles", "diploid_rate.txt"), help="the file the lines are appended to")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    L = m.load_library()
    n = a.mb << 20
    g0 = torch.Generator(device="cuda").manual_seed(20261018)
    world = torch.randint(0, 4, (n,), generator=g0, device="cuda", dtype=torch.uint8)
    nreads = int(a.cov * n / a.len)
    out_dir = a.out or tempfile.mkdtemp(prefix="mfx_diploid_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    fr, f1, f2, fm = (os.path.join(out_dir, x) for x in ("reads.mfxk", "hap1.mfxk", "hap2.mfxk", "merged.mfxk"))
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    try:
        kmers, n_read, secs = _count_half(torch, m, L, world, a, nreads, 7, fr)
        say("k=%d genome=%d Mb: %d reads x %d bases (%.0fx, %.3f %% substitutions) counted in %.1f s: %.3f G k-mers, %.3f G distinct, file %.2f GB in %s"
            % (a.k, a.mb, nreads, a.len, a.cov, 100 * a.err, secs, kmers / 1e9, n_read / 1e9, os.path.getsize(fr) / 1e9, out_dir))
        n1, secs = _count_genome(torch, m, L, world, a.k, f1)
        say("hap1 (the genome as one record) counted in %.1f s: %.3f G distinct, file %.2f GB" % (secs, n1 / 1e9, os.path.getsize(f1) / 1e9))
        at = torch.arange(a.every // 2, n, a.every, device="cuda")
        world[at] = (world[at] + 1 + (at % 3).to(torch.uint8)) & 3      # another base at each of these positions
        n2, secs = _count_genome(torch, m, L, world, a.k, f2)
        say("hap2 (a substitution every %d bases: a placeholder density) counted in %.1f s: %.3f G distinct, file %.2f GB" % (a.every, secs, n2 / 1e9, os.path.getsize(f2) / 1e9))
        del world
        torch.cuda.empty_cache()
        os.environ["MFX_DB_TIMING"] = "1"
        kp = m.KParams(a.peak)

        def diploid():
            t0 = time.time()
            r = m.db_diploid(fr, f1, f2, copies=4, max_mult=10000, kparams=kp)
            return r, time.time() - t0

        def chain():
            t0 = time.time()
            parts = {}
            m.db_merge([f1, f2], fm)
            parts["merge"] = time.time() - t0
            tu = []
            for name, fa in (("hap1", f1), ("hap2", f2), ("both", fm)):
                t1 = time.time()
                tu.append(m.db_join_completeness(fr, fa, kp, with_stats=True))
                parts["completeness " + name] = time.time() - t1
            t1 = time.time()
            img, entries, ss = m.db_join_spectrum(fr, fm, 4, 10000, with_entries=True, with_stats=True)
            parts["spectrum"] = time.time() - t1
            return (tu, img, entries, ss, parts), time.time() - t0

        # ---- all outputs equal before anything is timed
        d, _ = diploid()
        (tu, img, entries, _, _), _ = chain()
        assert np.array_equal(d["cn_img"], img) and d["n_entries"] == entries, "the cn images differ"
        for i in range(3):
            assert np.array_equal(d["total"], tu[i][0]) and np.array_equal(d["undrcpy"][i], tu[i][1]), "the piece sums differ"
        assert np.array_equal(d["asm_img"].sum(axis=0), d["cn_img"].sum(axis=0))
        st = d["stats"]
        say("outputs equal on both legs: %d entries; hap1 / hap2 / both distinct %d / %d / %d, of them not in the reads %d / %d / %d; %d in both assemblies; %d windows"
            % (d["n_entries"], st["hap1"]["distinct"], st["hap2"]["distinct"], st["both"]["distinct"], st["hap1"]["only_distinct"], st["hap2"]["only_distinct"],
               st["both"]["only_distinct"], st["n_shared"], st["windows"]))
        secs = {"diploid": [], "chain": []}
        for rep in range(a.reps):
            d, tw = diploid()
            s = d["stats"]
            secs["diploid"].append(tw)
            say("rep %d  diploid %.2f s = pread + copy %.2f s + decode %.3f s + pair run %.3f s + join %.3f s + the rest %.2f s"
                % (rep, tw, s["t_read"], s["t_decode"], s["t_pair"], s["t_join"], s["t_total"] - s["t_read"] - s["t_decode"] - s["t_pair"] - s["t_join"]))
            (tu, _, _, ss, parts), tw = chain()
            secs["chain"].append(tw)
            reads = sum(x[2]["t_read"] for x in tu) + ss["t_read"]
            say("rep %d  chain   %.2f s = %s   (pread + copy of the four joins %.2f s)" % (rep, tw, " + ".join("%s %.2f s" % kv for kv in parts.items()), reads))
        say("diploid %s s; chain %s s" % (", ".join("%.2f" % x for x in secs["diploid"]), ", ".join("%.2f" % x for x in secs["chain"])))
        apart = max(secs["diploid"]) < min(secs["chain"])
        say("the ranges %s" % ("lie apart, the one call below the chain" if apart else "overlap, or the one call is not below the chain"))
    finally:
        for x in (fr, f1, f2, fm):
            if os.path.exists(x):
                os.remove(x)
        os.makedirs(os.path.dirname(os.path.abspath(a.profile)), exist_ok=True)
        with open(a.profile, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
