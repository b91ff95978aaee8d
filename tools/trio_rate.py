"""Rates of mfx_db_trio against the only route there was before it: the chain of five mfx_db_merge / mfx_db_merge_except calls.

Three databases are made as tools/count_rate.py makes its one: a seeded i.i.d. genome of --mb Mb on the device is the mother's haplotype;
the father's is the same genome with a substitution every --het bases; reads of --len bases at --cov x, both strands, substitutions at
--err per base, are drawn from the mother's haplotype (mat), the father's (pat) and half and half from both (child), counted by the
claiming counter and written as sorted databases.  The heterozygosity and the i.i.d. genome are placeholders: real parents differ by
indels and structure too, and a real genome repeats.

First the three routes run once and their outputs are compared byte for byte (the explicit cutoffs are the ones the automatic route
reports).  Then, in one visit, alternating, --reps times each:
  (a) db_trio with explicit cutoffs (one pass);
  (b) db_trio with automatic cutoffs (the histogram pass, then the same pass);
  (c) the chain: db_merge_except(mat, pat, min), db_merge_except(pat, mat, min), db_merge(child, min), two db_merge intersect.
Per run: the seconds, and for db_trio the read / decode / merge / histogram / classify / writer / close seconds of its stats (MFX_DB_TIMING
is set, so the kernels' times are their own).  The lines go to stdout and are appended to --profile (default profiles/trio_rate.txt).
No threshold is set on any of this.

    python tools/trio_rate.py [--mb 256] [--cov 30] [--len 150] [--err 0.005] [--het 1000] [--k 21] [--reps 5] [--out DIR] [--profile FILE]
"""
import argparse
import ctypes as C
import filecmp
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.count_rate import _read_chunk      # noqa: E402


def _count(torch, m, L, a, parts, path):
    """the reads of parts = [(world, nreads, seed)] counted into one table created small, the table written to `path`; (k-mers, distinct, seconds)"""
    from merfin_amd.binding import _ReadsStats
    t0 = time.time()
    ix = m.Index(a.k, 1024)
    r = L.mfx_reads_begin_all(ix.h, 0)
    assert r, L.mfx_last_error()
    for world, nreads, seed in parts:
        g = torch.Generator(device="cuda").manual_seed(seed)
        done = 0
        while done < nreads:
            c = min(1 << 20, nreads - done)
            host = _read_chunk(torch, world, c, a.len, a.err, g).cpu().numpy()
            ptrs = (C.c_char_p * c).from_buffer_copy(np.arange(c, dtype=np.uint64) * a.len + host.ctypes.data)
            lens = np.full(c, a.len, dtype=np.uint64)
            assert L.mfx_reads_add(r, ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)), c) == 0, L.mfx_last_error()
            done += c
    st = _ReadsStats()
    assert L.mfx_reads_end(r, C.byref(st)) == 0, L.mfx_last_error()
    n = ix.write_db(path, 0, streamed=True)
    ix.close()
    return st.kmers, n, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--cov", type=float, default=30.0)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--het", type=int, default=1000, help="the father's haplotype differs from the mother's by one substitution every this many bases")
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maxmult", type=int, default=10000)
    ap.add_argument("--out", default=None, help="directory of the databases (default: tmpfs)")
    ap.add_argument("--profile", default=os.path.join(ROOT, "profiles", "trio_rate.txt"), help="the file the lines are appended to")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    L = m.load_library()
    n = a.mb << 20
    g0 = torch.Generator(device="cuda").manual_seed(20261021)
    mat_w = torch.randint(0, 4, (n,), generator=g0, device="cuda", dtype=torch.uint8)
    pat_w = mat_w.clone()
    at = torch.arange(a.het // 2, n, a.het, device="cuda")
    pat_w[at] = (pat_w[at] + torch.randint(1, 4, (len(at),), generator=g0, device="cuda", dtype=torch.uint8)) % 4
    nreads = int(a.cov * n / a.len)
    out_dir = a.out or tempfile.mkdtemp(prefix="mfx_trio_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    p = {x: os.path.join(out_dir, x + ".mfxk") for x in ("mat", "pat", "child", "A", "B", "A2", "B2", "x", "y", "z", "cA", "cB")}
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def trio(cuts, oa, ob):
        t0 = time.time()
        st = m.db_trio(p["mat"], p["pat"], p["child"], oa, ob, cut_mat=cuts[0], cut_pat=cuts[1], cut_child=cuts[2], max_mult=a.maxmult)
        return st, time.time() - t0

    def chain(cuts):
        t0 = time.time()
        m.db_merge_except([p["mat"]], [p["pat"]], p["x"], min_count=cuts[0])
        m.db_merge_except([p["pat"]], [p["mat"]], p["z"], min_count=cuts[1])
        m.db_merge([p["child"]], p["y"], min_count=cuts[2])
        m.db_merge([p["x"], p["y"]], p["cA"], op="intersect")
        m.db_merge([p["z"], p["y"]], p["cB"], op="intersect")
        return time.time() - t0

    def split(st):
        return "read %.2f, decode %.2f, merge %.2f, hist %.2f, classify %.2f, writers %.2f, close %.2f s" % tuple(
            st[x] for x in ("t_read", "t_decode", "t_merge", "t_hist", "t_classify", "t_write", "t_close"))
    try:
        for name, parts in (("mat", [(mat_w, nreads, 7)]), ("pat", [(pat_w, nreads, 8)]), ("child", [(mat_w, nreads // 2, 9), (pat_w, nreads - nreads // 2, 10)])):
            kmers, distinct, secs = _count(torch, m, L, a, parts, p[name])
            say("k=%d genome=%d Mb, pat = mat with a substitution every %d bases: %-5s %d reads x %d bases (%.0fx, %.3f %% substitutions) counted in %.1f s: "
                "%.3f G k-mers, %.3f G distinct, file %.2f GB in %s" % (a.k, a.mb, a.het, name, sum(x[1] for x in parts), a.len, a.cov, 100 * a.err, secs, kmers / 1e9,
                                                                       distinct / 1e9, os.path.getsize(p[name]) / 1e9, out_dir))
        del mat_w, pat_w
        torch.cuda.empty_cache()
        os.environ["MFX_DB_TIMING"] = "1"
        devnull = os.open(os.devnull, os.O_WRONLY)               # (what MFX_DB_TIMING prints per writer is not kept: the stats hold the split)
        keep = os.dup(2)
        os.dup2(devnull, 2)
        try:
            # ---- the outputs of the three routes, byte for byte, before anything is timed
            st, _ = trio((0, 0, 0), p["A"], p["B"])
            cuts = (st["cut_mat"], st["cut_pat"], st["cut_child"])
            say("automatic cutoffs: mat %d, pat %d, child %d; %.3f G k-mers of both parents, %.3f G of mat alone (%.3f G at the cutoff), %.3f G of pat alone (%.3f G); "
                "A %.3f G, B %.3f G k-mers; %d windows" % (cuts + (st["n_both"] / 1e9, st["n_mat_only"] / 1e9, st["n_mat_only_cut"] / 1e9, st["n_pat_only"] / 1e9,
                                                          st["n_pat_only_cut"] / 1e9, st["n_a"] / 1e9, st["n_b"] / 1e9, st["windows"])))
            trio(cuts, p["A2"], p["B2"])
            chain(cuts)
            same = all(filecmp.cmp(p[x], p[y], shallow=False) for x, y in (("A", "A2"), ("B", "B2"), ("A", "cA"), ("B", "cB")))
            say("the outputs of db_trio (automatic), db_trio (explicit) and the chain are %s (A %.2f GB, B %.2f GB; the chain's intermediate files %.2f GB)"
                % ("equal, byte for byte" if same else "DIFFERENT", os.path.getsize(p["A"]) / 1e9, os.path.getsize(p["B"]) / 1e9,
                   sum(os.path.getsize(p[x]) for x in "xyz") / 1e9))
            assert same
            secs = {"explicit": [], "auto": [], "chain": []}
            for rep in range(a.reps):
                st, tw = trio(cuts, p["A2"], p["B2"])
                secs["explicit"].append(tw)
                say("rep %d  trio explicit %.2f s  (%s)" % (rep, tw, split(st)))
                st, tw = trio((0, 0, 0), p["A"], p["B"])
                secs["auto"].append(tw)
                say("rep %d  trio auto     %.2f s  (%s)" % (rep, tw, split(st)))
                tw = chain(cuts)
                secs["chain"].append(tw)
                say("rep %d  chain         %.2f s" % (rep, tw))
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            os.close(devnull)
        for kind in ("explicit", "auto", "chain"):
            say("%-8s %s s (%.2f to %.2f)" % (kind, ", ".join("%.2f" % x for x in secs[kind]), min(secs[kind]), max(secs[kind])))
        for kind in ("explicit", "auto"):
            apart = max(secs[kind]) < min(secs["chain"])
            say("trio %s against the chain: the ranges %s" % (kind, "lie apart, the trio below" if apart else "overlap, or the trio is not below"))
    finally:
        for x in p.values():
            if os.path.exists(x):
                os.remove(x)
        os.makedirs(os.path.dirname(os.path.abspath(a.profile)), exist_ok=True)
        with open(a.profile, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
