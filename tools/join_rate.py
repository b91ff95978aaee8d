"""Rates of mfx_db_join_* against the only route there was before it: both databases loaded into one full table, then
mfx_completeness_pieces and mfx_spectrum_run on the table.

The world of tools/merge_rate.py (a seeded i.i.d. genome of --mb Mb generated on the device, reads of --len bases at --cov x, both
strands, substitutions at --err per base).  The read database comes from the claiming counter over the reads, the assembly's database
from the same counter over the genome as one record; both are written as sorted flat files into tmpfs.  Then, in one visit, alternating,
--reps times each, the whole call from the files:
  (a) table: a full table sized for both files, load_db of both, completeness_pieces + spectrum;
  (b) join:  db_join_completeness + db_join_spectrum, with MFX_DB_TIMING set so that the join kernel is waited for per window and the
      split (pread + copy, decode, join kernel, the rest) is the library's own;
  (c) merge: db_merge of the two files (sum), for its MFX_DB_TIMING line: what mfx_merge_pairs_kernel + mfx_combine_kernel take on the
      same two runs (printed to 0.01 s by the library).
The results of (a) and (b) must be equal.  The lines go to stdout and are appended to --profile (default profiles/join_rate.txt).  No
threshold is set on any of this.

    python tools/join_rate.py [--mb 256] [--cov 30] [--len 150] [--err 0.005] [--k 21] [--reps 5] [--out DIR] [--profile FILE]
"""
import argparse
import ctypes as C
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.count_rate import _with_stderr      # noqa: E402
from tools.merge_rate import _count_half       # noqa: E402


def _count_genome(torch, m, L, world, k, path):
    """the genome as one record through the claiming counter, the table written to `path`; (distinct k-mers, seconds)"""
    from merfin_amd.binding import _ReadsStats
    t0 = time.time()
    ix = m.Index(k, 1024)
    r = L.mfx_reads_begin_all(ix.h, 0)
    assert r, L.mfx_last_error()
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    host = lut[world.long()].cpu().numpy()
    ptrs = (C.c_char_p * 1).from_buffer_copy(np.array([host.ctypes.data], dtype=np.uint64))
    lens = np.array([len(host)], dtype=np.uint64)
    assert L.mfx_reads_add(r, ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)), 1) == 0, L.mfx_last_error()
    st = _ReadsStats()
    assert L.mfx_reads_end(r, C.byref(st)) == 0, L.mfx_last_error()
    n = ix.write_db(path, 0, streamed=True)
    ix.close()
    return n, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--cov", type=float, default=30.0)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--peak", type=float, default=26.0)
    ap.add_argument("--out", default=None, help="directory of the databases (default: tmpfs)")
    ap.add_argument("--profile", default=os.path.join(ROOT, "profiles", "join_rate.txt"), help="the file the lines are appended to")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    L = m.load_library()
    n = a.mb << 20
    g0 = torch.Generator(device="cuda").manual_seed(20261018)
    world = torch.randint(0, 4, (n,), generator=g0, device="cuda", dtype=torch.uint8)
    nreads = int(a.cov * n / a.len)
    out_dir = a.out or tempfile.mkdtemp(prefix="mfx_join_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    fr, fa, fm = (os.path.join(out_dir, x) for x in ("reads.mfxk", "asm.mfxk", "merged.mfxk"))
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    try:
        kmers, n_read, secs = _count_half(torch, m, L, world, a, nreads, 7, fr)
        say("k=%d genome=%d Mb: %d reads x %d bases (%.0fx, %.3f %% substitutions) counted in %.1f s: %.3f G k-mers, %.3f G distinct, file %.2f GB in %s"
            % (a.k, a.mb, nreads, a.len, a.cov, 100 * a.err, secs, kmers / 1e9, n_read / 1e9, os.path.getsize(fr) / 1e9, out_dir))
        n_asm, secs = _count_genome(torch, m, L, world, a.k, fa)
        say("the assembly (the genome as one record) counted in %.1f s: %.3f G distinct, file %.2f GB" % (secs, n_asm / 1e9, os.path.getsize(fa) / 1e9))
        del world
        torch.cuda.empty_cache()
        os.environ["MFX_DB_TIMING"] = "1"
        kp = m.KParams(a.peak)
        secs = {"table": [], "join": []}
        kernel = {"join": [], "merge": []}
        first = None
        for rep in range(a.reps):
            for kind in ("table", "join", "merge"):
                def run():
                    t0 = time.time()
                    if kind == "table":
                        ix = m.Index(a.k, n_read + n_asm)      # (the union is not known before the load: sized for no k-mer shared)
                        ix.load_db(fr, 0)
                        ix.load_db(fa, 1)
                        t1 = time.time()
                        t, u = m.Evaluator(ix, kp).completeness_pieces()
                        t2 = time.time()
                        img = ix.spectrum(4, 10000)
                        t3 = time.time()
                        ix.close()
                        return (t, u, img), {"load": t1 - t0, "completeness": t2 - t1, "spectrum": t3 - t2}, time.time() - t0
                    if kind == "join":
                        t, u, sc = m.db_join_completeness(fr, fa, kp, with_stats=True)
                        img, ss = m.db_join_spectrum(fr, fa, 4, 10000, with_stats=True)
                        return (t, u, img), {"completeness": sc, "spectrum": ss}, time.time() - t0
                    st = m.db_merge([fr, fa], fm)
                    return None, st, time.time() - t0
                (res, what, tw), err = _with_stderr(run)
                if kind == "merge":
                    for x in err.splitlines():
                        if x.startswith("[mfx db] merge"):
                            say("rep %d  merge %.2f s        %s" % (rep, tw, x))
                            g = re.search(r"merge ([0-9.]+) s, combine ([0-9.]+) s", x)
                            if g:
                                kernel["merge"].append((float(g.group(1)) + float(g.group(2))) / (n_read + n_asm))
                    continue
                if first is None:
                    first = res
                same = all(np.array_equal(x, y) for x, y in zip(res, first))
                assert same, "the routes differ"
                secs[kind].append(tw)
                if kind == "table":
                    say("rep %d  table %.2f s = load_db of both %.2f s + completeness %.3f s + spectrum %.3f s + release" % (rep, tw, what["load"], what["completeness"], what["spectrum"]))
                else:
                    for name in ("completeness", "spectrum"):
                        s = what[name]
                        rest = s["t_total"] - s["t_read"] - s["t_decode"] - s["t_join"]
                        recs = s["n_read"] + s["n_asm"]
                        kernel["join"].append(s["t_join"] / recs)
                        say("rep %d  join  %-12s %.2f s = pread + copy %.2f s + decode %.3f s + join kernel %.4f s + the rest %.2f s   (%d windows, %.3f G records, %.3f G in both; "
                            "the kernel: %.1f G records/s = %.1f GB/s of the 12 bytes a record)"
                            % (rep, name, s["t_total"], s["t_read"], s["t_decode"], s["t_join"], rest, s["windows"], recs / 1e9, s["n_both"] / 1e9,
                               recs / max(s["t_join"], 1e-9) / 1e9, 12 * recs / max(s["t_join"], 1e-9) / 1e9))
                    say("rep %d  join  both reports %.2f s" % (rep, tw))
        say("results equal on both routes in every repetition")
        say("table %s s; join %s s" % (", ".join("%.2f" % x for x in secs["table"]), ", ".join("%.2f" % x for x in secs["join"])))
        apart = max(secs["join"]) < min(secs["table"])
        say("the ranges %s" % ("lie apart, the join below" if apart else "overlap, or the join is not below"))
        if kernel["merge"] and kernel["join"]:
            jk, mk = sorted(kernel["join"]), sorted(kernel["merge"])
            say("per record: join kernel %.3f .. %.3f ns; merge_pairs + combine %.3f .. %.3f ns (from a line printed to 0.01 s)" % (jk[0] * 1e9, jk[-1] * 1e9, mk[0] * 1e9, mk[-1] * 1e9))
    finally:
        for x in (fr, fa, fm):
            if os.path.exists(x):
                os.remove(x)
        os.makedirs(os.path.dirname(os.path.abspath(a.profile)), exist_ok=True)
        with open(a.profile, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
