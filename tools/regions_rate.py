"""Rate of `-regions` (mfx_regions_run: class planes, runs by count / scan / scatter, a second pass for the sums) on the device, against
`-track` at W = 1000 on the same index and against the route the same intervals took before: mfx_dump_values over every contig
(8 bytes per position over the link) plus the numpy pipeline of tests/regions_ref.py on the host.

A seeded synthetic world of --mb Mb (tools/synth_torch.py, generated on the device) with the sequence-only compact index at
k = 21, as `merfin -regions` builds it; then the `repeats` world at its 3 % level, where far more tiles hold a flagged position.
In ONE process, alternating the legs --reps times after a warm-up of each:
  regions     : wall time of Evaluator.regions(seqs) at the defaults (kstar 1.0, gap 0, min_kmers 1) -- allocations, both passes, the
                scans and the copy of the records to the host included -- as k-mers (valid start positions) per second; beside it
                what the library timed inside the call: pass 1, runs / joining / filter, pass 2 (each waited for);
  track       : wall time of Evaluator.track(seqs, 1000) on the same evaluator;
  dump route  : Evaluator.dump_values of every contig + regions_ref's class masks, runs, joining and sums in numpy.
Every leg ends in a device synchronise (the calls return host arrays).  The records of the device path are compared with the dump
route's, every field, before anything is timed.  No bar is set on a rate: where two ranges overlap the tool says so.

    python tools/regions_rate.py [--mb 256] [--reps 5] [--out profiles/regions_rate.txt] [--commit ID]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump_route(m, rr, ev, kp, seqs, lens, t, gap, min_kmers):
    """the records from the raw per-position values (what a caller of the C ABI could do before); returns them and the device's share of the time"""
    pp = []
    t_dev = 0.0
    for c, n in enumerate(lens):
        t0 = time.perf_counter()
        rv, av, ka, km = ev.dump_values(seqs, c, 0, n) if n else (np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0, 0)
        t_dev += time.perf_counter() - t0
        valid = av != 0                                          # a valid k-mer has asmV >= 1 on this index (the assembly's own counts)
        top = int(rv.max()) if n else 0
        if top < (1 << 20):                                      # readK of every read count up to the largest one met: a table
            rk = np.array([m.getK(kp, v, 0)[0] for v in range(top + 1)])[rv]
        else:
            u, inv = np.unique(rv, return_inverse=True)
            rk = np.array([m.getK(kp, int(v), 0)[0] for v in u.tolist()])[inv]
        ak = av.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ks = np.where(ak > rk, -(ak / rk - 1), np.where(ak < rk, rk / ak - 1, 0.0))
        ks = np.where(valid & (rk != 0), ks, 0.0)
        pp.append((valid, rk, ak, ks))
    return rr.regions(pp, t, gap, min_kmers), t_dev


def measure(m, rr, st, say, mb, reps, repeats):
    k, lam = 21, 26.0
    ix, seqs, asm, info = st.build_world(m, mb << 20, k=k, lam=lam, ncontigs=24, seq_only=True, repeats=repeats)
    lens = [int(x.numel()) for x in asm]
    kp = m.KParams.from_file(lam, os.path.join(ROOT, "tests", "golden", "example_lookup_table.txt"))
    ev = m.Evaluator(ix, kp)
    ntiles = sum((n + 4095) // 4096 for n in lens)
    say("world: %d Mb synthetic (tools/synth_torch.py%s), %d contigs, %d tiles, k = %d, sequence-only index (compact = %s), -prob table of 184 rows"
        % (mb, ", repeats level %d" % repeats if repeats else "", len(lens), ntiles, k, info.get("compact")))
    h = ev.hist(seqs)
    kasm = h.kasm
    t_dump, t_dump_dev = [], []
    got, ka, km, revisited = ev.regions(seqs)
    ev.track(seqs, 1000)
    t0 = time.perf_counter()
    want, td = dump_route(m, rr, ev, kp, seqs, lens, 1.0, 0, 1)
    t_dump.append(time.perf_counter() - t0)
    t_dump_dev.append(td)
    assert (ka, km) == (h.kasm, h.kmissing)
    assert rr.same_records(got, want) is None, rr.same_records(got, want)
    per_cls = [int((got["cls"] == c).sum()) for c in range(3)]
    say("records of the device path == the dump route's, every field: %d records (missing %d, collapsed %d, expanded %d), %d flagged k-mers"
        % (len(got), per_cls[0], per_cls[1], per_cls[2], int(got["n_kmers"].sum())))
    say("tiles pass 2 evaluated: %d of %d = %.4f" % (revisited, ntiles, revisited / max(ntiles, 1)))
    t_reg, t_trk, parts = [], [], []
    for rep in range(reps):
        ms = []
        t0 = time.perf_counter()
        ev.regions(seqs, times=ms)
        t_reg.append(time.perf_counter() - t0)
        parts.append(ms)
        t0 = time.perf_counter()
        ev.track(seqs, 1000)
        t_trk.append(time.perf_counter() - t0)
        if rep + 1 < reps:                                       # (the check above was the dump route's first run)
            t0 = time.perf_counter()
            _, td = dump_route(m, rr, ev, kp, seqs, lens, 1.0, 0, 1)
            t_dump.append(time.perf_counter() - t0)
            t_dump_dev.append(td)
    rate = lambda s: kasm / s / 1e9
    rng = lambda v: "%.3f - %.3f G k-mers/s" % (rate(max(v)), rate(min(v)))
    say("k-mers (valid start positions): %d" % kasm)
    say("regions     : %.2f - %.2f ms (%d runs) = %s" % (min(t_reg) * 1e3, max(t_reg) * 1e3, len(t_reg), rng(t_reg)))
    p = np.array(parts)
    say("  inside    : pass 1 %.2f - %.2f ms, runs / joining / filter %.2f - %.2f ms, pass 2 %.2f - %.2f ms"
        % (p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max(), p[:, 2].min(), p[:, 2].max()))
    say("track W=1000: %.2f - %.2f ms (%d runs) = %s" % (min(t_trk) * 1e3, max(t_trk) * 1e3, len(t_trk), rng(t_trk)))
    say("dump route  : %.1f - %.1f ms (%d runs), of which mfx_dump_values %.1f - %.1f ms (8 B per position to the host) = %s"
        % (min(t_dump) * 1e3, max(t_dump) * 1e3, len(t_dump), min(t_dump_dev) * 1e3, max(t_dump_dev) * 1e3, rng(t_dump)))
    if max(t_reg) < min(t_dump):
        say("  the ranges of regions and of the dump route do not overlap: regions is %.0f - %.0fx faster" % (min(t_dump) / max(t_reg), max(t_dump) / min(t_reg)))
    else:
        say("  the ranges of regions and of the dump route OVERLAP: no speed-up is claimed")
    if max(p[:, 0]) < min(t_trk) * 1e3 or min(p[:, 0]) > max(t_trk) * 1e3:
        say("  pass 1 against track W=1000: the ranges do not overlap, pass 1 takes %.2f - %.2f of track's time" % (p[:, 0].min() / (max(t_trk) * 1e3), p[:, 0].max() / (min(t_trk) * 1e3)))
    else:
        say("  pass 1 against track W=1000: the ranges overlap")
    del ev, seqs, ix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the tree was built from, where the tree is not a git checkout")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    from tests import regions_ref as rr
    from tools import synth_torch as st
    if m.device_count() < 1:
        raise SystemExit("regions_rate: no HIP device visible; the rate is measured on the GPU or not at all")
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
    say("regions_rate: %s, %s; commit %s" % (torch.cuda.get_device_name(0), m.load_library().mfx_version().decode(), commit))
    say("Evaluator.regions at kstar 1.0, gap 0, min_kmers 1; %d runs of each leg, alternating" % a.reps)
    for repeats in (0, 3):
        measure(m, rr, st, say, a.mb, a.reps, repeats)
        if a.out:                                                # (what is measured so far is kept)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
