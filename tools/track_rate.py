"""Rate of `-track` (mfx_track_run, mfx_track_kernel) on the device, against the -hist kernel on the same index and against
the route the same answer took before: mfx_dump_values over every contig (8 bytes per position over the link) plus a window
reduction on the host.

A seeded synthetic world of --mb Mb (tools/synth_torch.py, generated on the device) with the sequence-only compact index at
k = 21, as `merfin -track` builds it.  In ONE process, alternating the legs --reps times after a warm-up of each:
  track W     : wall time of Evaluator.track(seqs, W) -- the records' allocation and clearing, the kernel, the min / max pass and
                the copy of the records to the host included -- as k-mers (valid start positions) per second;
  hist        : wall time of Evaluator.hist(seqs) on the same evaluator;
  dump route  : Evaluator.dump_values of every contig + a numpy reduction per window (readK through a table of the distinct
                read counts, K*, counts, sums, min, max; its sum of K* is a float64 sum, not the exact integer).
Every leg ends in a device synchronise (the calls return host arrays).  The records of the fused path are checked against the
dump route's counts and sums at every W before anything is timed.

    python tools/track_rate.py [--mb 256] [--reps 5] [--windows 100,1000,100000] [--out profiles/track_windows.txt] [--commit ID]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump_route(m, ev, kp, seqs, lens, W):
    """the window records' integer fields, min and max from the raw per-position values (what a caller of the C ABI could do before)"""
    cols = {f: [] for f in ("n_kmers", "n_missing", "n_scored", "n_pos", "n_neg", "sum_readK", "sum_asmK", "sum", "min", "max")}
    t_dev = 0.0
    for c, n in enumerate(lens):
        if n == 0:
            continue
        t = time.perf_counter()
        rv, av, ka, km = ev.dump_values(seqs, c, 0, n)
        t_dev += time.perf_counter() - t
        # a valid k-mer has asmV >= 1 on this index (the assembly's own counts): validity = asmV != 0
        valid = av != 0
        top = int(rv.max())
        if top < (1 << 20):                                      # readK of every read count up to the largest one met: a table
            rk = np.array([m.getK(kp, v, 0)[0] for v in range(top + 1)])[rv]
        else:
            u, inv = np.unique(rv, return_inverse=True)
            rk = np.array([m.getK(kp, int(v), 0)[0] for v in u.tolist()])[inv]
        ak = av.astype(np.float64)
        missing = valid & (rk == 0)
        scored = valid & ~missing
        with np.errstate(divide="ignore", invalid="ignore"):
            ks = np.where(ak > rk, -(ak / rk - 1), np.where(ak < rk, rk / ak - 1, 0.0))
        ks = np.where(scored, ks, 0.0)
        starts = np.arange(0, n, W, dtype=np.int64)
        red = lambda a: np.add.reduceat(a.astype(np.uint64), starts)
        cols["n_kmers"].append(red(valid))
        cols["n_missing"].append(red(missing))
        cols["n_scored"].append(red(scored))
        cols["n_pos"].append(red(ks > 0))
        cols["n_neg"].append(red(ks < 0))
        cols["sum_readK"].append(red(np.where(scored, rk, 0)))
        cols["sum_asmK"].append(red(np.where(scored, av, 0)))
        cols["sum"].append(np.add.reduceat(ks, starts))
        cols["min"].append(np.minimum.reduceat(np.where(scored, ks, np.inf), starts))
        cols["max"].append(np.maximum.reduceat(np.where(scored, ks, -np.inf), starts))
    return {f: np.concatenate(v) for f, v in cols.items()}, t_dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", default="100,1000,100000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the tree was built from, where the tree is not a git checkout")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    from tools import synth_torch as st
    if m.device_count() < 1:
        raise SystemExit("track_rate: no HIP device visible; the rate is measured on the GPU or not at all")
    k, lam = 21, 26.0
    total = a.mb << 20
    windows = [int(x) for x in a.windows.split(",")]
    ix, seqs, asm, info = st.build_world(m, total, k=k, lam=lam, ncontigs=24, seq_only=True)
    lens = [int(x.numel()) for x in asm]
    kp = m.KParams.from_file(lam, os.path.join(ROOT, "tests", "golden", "example_lookup_table.txt"))
    ev = m.Evaluator(ix, kp)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    commit = a.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    commit = commit or "unknown (not a git checkout)"
    say("track_rate: %s, %s; commit %s" % (torch.cuda.get_device_name(0), m.load_library().mfx_version().decode(), commit))
    say("world: %d Mb synthetic (tools/synth_torch.py), %d contigs, k = %d, sequence-only index (compact = %s), -prob table of 184 rows"
        % (a.mb, len(lens), k, info.get("compact")))
    h = ev.hist(seqs)
    kasm = h.kasm
    # correctness before speed: the fused records against the dump route, every W
    t_track = {W: [] for W in windows}
    t_hist, t_dump, t_dump_dev = [], {W: [] for W in windows}, {W: [] for W in windows}
    for W in windows:
        w, ka, km = ev.track(seqs, W)
        t = time.perf_counter()
        ref, td = dump_route(m, ev, kp, seqs, lens, W)
        t_dump[W].append(time.perf_counter() - t)               # (the slow leg is timed here and once more below)
        t_dump_dev[W].append(td)
        assert (ka, km) == (h.kasm, h.kmissing)
        for f in ("n_kmers", "n_missing", "n_scored", "n_pos", "n_neg", "sum_readK", "sum_asmK"):
            assert np.array_equal(w[f].astype(np.uint64), ref[f]), (W, f)
        assert np.array_equal(w["min_kstar"], ref["min"]) and np.array_equal(w["max_kstar"], ref["max"]), W
        exact = (w["sum_kstar_hi"].astype(np.float64) * 2.0 ** 64 + w["sum_kstar_lo"].astype(np.float64)) / 2.0 ** 52
        assert np.allclose(exact, ref["sum"], rtol=1e-9, atol=1e-9), W
    say("records of the fused path == the dump route's (counts, sums, min, max; float sum of K* to 1e-9) at W = %s" % windows)
    # (the check above warmed every shape up) the timed legs alternate
    for rep in range(a.reps):
        for W in windows:
            t = time.perf_counter()
            ev.track(seqs, W)
            t_track[W].append(time.perf_counter() - t)
        t = time.perf_counter()
        ev.hist(seqs)
        t_hist.append(time.perf_counter() - t)
        if rep == 0:
            for W in windows:
                t = time.perf_counter()
                _, td = dump_route(m, ev, kp, seqs, lens, W)
                t_dump[W].append(time.perf_counter() - t)
                t_dump_dev[W].append(td)
    med = lambda v: float(np.median(v))
    rate = lambda s: kasm / s / 1e9
    say("k-mers (valid start positions): %d" % kasm)
    say("hist        : median %.2f ms (min %.2f, max %.2f; %d runs) = %.2f G k-mers/s  [Evaluator.hist wall: launch + image copy]"
        % (med(t_hist) * 1e3, min(t_hist) * 1e3, max(t_hist) * 1e3, len(t_hist), rate(med(t_hist))))
    for W in windows:
        nrec = m.load_library().mfx_track_num_windows(seqs.h, W)
        say("track W=%-7d: median %.2f ms (min %.2f, max %.2f; %d runs) = %.2f G k-mers/s; %d records (%.1f MB to the host); ratio to hist %.3f"
            % (W, med(t_track[W]) * 1e3, min(t_track[W]) * 1e3, max(t_track[W]) * 1e3, len(t_track[W]), rate(med(t_track[W])), nrec, nrec * 72 / 1e6,
               med(t_hist) / med(t_track[W])))
        say("dump  W=%-7d: median %.1f ms (%d runs), of which mfx_dump_values %.1f ms (8 B per position to the host), numpy reduction %.1f ms = %.3f G k-mers/s; "
            "fused path %.1fx faster" % (W, med(t_dump[W]) * 1e3, len(t_dump[W]), med(t_dump_dev[W]) * 1e3, (med(t_dump[W]) - med(t_dump_dev[W])) * 1e3,
                                         rate(med(t_dump[W])), med(t_dump[W]) / med(t_track[W])))
        assert med(t_track[W]) < med(t_dump[W]), "the fused path is not faster than the dump route at W = %d" % W
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
