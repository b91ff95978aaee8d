"""Rates of mfx_db_merge against the only route there was before it: both databases loaded into one full table, the table written as a
sorted database (write_db(streamed=True)).

The reads of tools/count_rate.py (a seeded i.i.d. genome of --mb Mb generated on the device, reads of --len bases at --cov x, both strands,
substitutions at --err per base) are cut in two halves; each half is counted by the claiming counter and written as a file of its own.
Then, in one visit, alternating, --reps times each:
  (a) db_merge of the two files (sum);
  (b) a full table sized for the union, load_db of both files into it, write_db(streamed=True).
The two outputs must be equal byte for byte.  Per run: the seconds, the k-mers per second read and written, and what MFX_DB_TIMING prints.
The lines go to stdout and are appended to --profile (default profiles/merge_rate.txt).  No threshold is set on any of this.

    python tools/merge_rate.py [--mb 256] [--cov 30] [--len 150] [--err 0.005] [--k 21] [--reps 3] [--out DIR] [--profile FILE]
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

from tools.count_rate import _read_chunk, _with_stderr      # noqa: E402


def _count_half(torch, m, L, world, a, nreads, seed, path):
    """nreads reads of the generator `seed` counted into a table created small, the table written to `path`; (k-mers, distinct, seconds)"""
    from merfin_amd.binding import _ReadsStats
    t0 = time.time()
    ix = m.Index(a.k, 1024)
    r = L.mfx_reads_begin_all(ix.h, 0)
    assert r, L.mfx_last_error()
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
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory of the databases (default: tmpfs)")
    ap.add_argument("--profile", default=os.path.join(ROOT, "profiles", "merge_rate.txt"), help="the file the lines are appended to")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    L = m.load_library()
    n = a.mb << 20
    g0 = torch.Generator(device="cuda").manual_seed(20261018)
    world = torch.randint(0, 4, (n,), generator=g0, device="cuda", dtype=torch.uint8)
    nreads = int(a.cov * n / a.len)
    out_dir = a.out or tempfile.mkdtemp(prefix="mfx_merge_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    fa, fb, out_a, out_b = (os.path.join(out_dir, x) for x in ("half_a.mfxk", "half_b.mfxk", "merged.mfxk", "table.mfxk"))
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    try:
        halves = []
        for path, seed, cnt in ((fa, 7, nreads // 2), (fb, 8, nreads - nreads // 2)):
            kmers, distinct, secs = _count_half(torch, m, L, world, a, cnt, seed, path)
            halves.append(distinct)
            say("k=%d genome=%d Mb: %d reads x %d bases (%.0fx in all, %.3f %% substitutions) counted in %.1f s: %.3f G k-mers, %.3f G distinct, file %.2f GB in %s"
                % (a.k, a.mb, cnt, a.len, a.cov, 100 * a.err, secs, kmers / 1e9, distinct / 1e9, os.path.getsize(path) / 1e9, out_dir))
        del world
        torch.cuda.empty_cache()
        n_in = sum(halves)
        os.environ["MFX_DB_TIMING"] = "1"
        secs = {"merge": [], "table": []}
        n_out = None
        for rep in range(a.reps):
            for kind in ("merge", "table"):
                def run():
                    t0 = time.time()
                    if kind == "merge":
                        st = m.db_merge([fa, fb], out_a)
                        return st["n_out"], st, time.time() - t0
                    ix = m.Index(a.k, n_in)                  # (the union is not known before the load: sized for no k-mer shared)
                    ix.load_db(fa, 0)
                    ix.load_db(fb, 0)
                    t1 = time.time()
                    nk = ix.write_db(out_b, 0, streamed=True)
                    t2 = time.time()
                    ix.close()
                    return nk, {"load": t1 - t0, "write": t2 - t1}, time.time() - t0
                (nk, what, tw), err = _with_stderr(run)
                assert n_out in (None, nk), (n_out, nk)
                n_out = nk
                secs[kind].append(tw)
                say("rep %d  %-5s %.3f G k-mers read, %.3f G written in %.2f s = %.1f M k-mers/s read, %.1f M k-mers/s written  %s"
                    % (rep, kind, n_in / 1e9, nk / 1e9, tw, n_in / tw / 1e6, nk / tw / 1e6,
                       ("(%d windows, %d saturated)" % (what["windows"], what["n_saturated"])) if kind == "merge"
                       else ("(load_db of both %.2f s, write_db %.2f s)" % (what["load"], what["write"]))))
                for x in err.splitlines():
                    if x.startswith("[mfx db] merge") or x.startswith("[mfx db] streamed"):
                        say("        " + x)
            if rep == 0:
                same = filecmp.cmp(out_a, out_b, shallow=False)
                say("rep 0  the two files are %s (%.2f GB)" % ("equal, byte for byte" if same else "DIFFERENT", os.path.getsize(out_a) / 1e9))
                assert same
        say("merge  %s s; table %s s" % (", ".join("%.2f" % x for x in secs["merge"]), ", ".join("%.2f" % x for x in secs["table"])))
        apart = max(secs["merge"]) < min(secs["table"])
        say("the ranges %s" % ("lie apart, the merge below" if apart else "overlap, or the merge is not below"))
    finally:
        for x in (fa, fb, out_a, out_b):
            if os.path.exists(x):
                os.remove(x)
        os.makedirs(os.path.dirname(os.path.abspath(a.profile)), exist_ok=True)
        with open(a.profile, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
