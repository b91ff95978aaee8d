"""Rate of `-phase` (mfx_phase_run: two haplotype planes, then markers -> runs -> blocks by count / scan / scatter) on the device, against
the only route to the same answer before it: mfx_dump_values over every contig (8 bytes per position over the link) plus the walk of
tests/phase_ref.py on the host; and its pass 1 beside pass 1 of `-regions` on the same index (mfx_diag_regions_times), a kernel that does
the same lookups and more arithmetic per position.

A seeded synthetic assembly of --mb Mb (tools/synth_torch.py, generated on the device), k = 21, the sequence-only compact index with the
assembly's k-mers claimed and two hap-mer sets loaded update-only: every position whose hash falls on 1 in --density is a marker; its
haplotype follows stretches of 50 000 positions, with an intrusion of the other haplotype over 2 000 positions in one stretch of 37 (the
density and the stretches are placeholders: no real trio was at hand).  In ONE process, alternating the legs --reps times after a
warm-up of each:
  phase       : wall time of Evaluator.phase(seqs) at the defaults (switches 100, range 20000) -- allocations, both passes, the scans and
                the copy of the records to the host included; beside it what the library timed inside: pass 1, runs / blocks;
  regions     : Evaluator.regions(seqs) on the same evaluator, for its pass 1;
  dump route  : Evaluator.dump_values of every contig + phase_ref's walk over the markers.
The records of the device path are compared with the dump route's, every field, before anything is timed.  No bar is set on a rate:
where two ranges overlap the tool says so.

    python tools/phase_rate.py [--mb 256] [--reps 5] [--density 100] [--out profiles/phase_rate.txt] [--commit ID]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump_route(pr, ev, seqs, lens, k, S, R):
    """the records from the raw per-position values; returns them, the marker counts and the device's share of the time"""
    markers, counts = [], []
    t_dev = 0.0
    for c, n in enumerate(lens):
        t0 = time.perf_counter()
        rv, av, _, _ = ev.dump_values(seqs, c, 0, n) if n else (np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0, 0)
        t_dev += time.perf_counter() - t0
        a, b = (rv != 0) & (av == 0), (av != 0) & (rv == 0)
        counts.append((int(a.sum()), int(b.sum()), int(((rv != 0) & (av != 0)).sum())))
        markers.append(pr.markers_of_masks(a, b))
    return pr.blocks(markers, k, S, R), counts, t_dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--density", type=int, default=100, help="one marker in this many positions")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the tree was built from, where the tree is not a git checkout")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    from tests import phase_ref as pr
    from tools import synth_torch as st
    if m.device_count() < 1:
        raise SystemExit("phase_rate: no HIP device visible; the rate is measured on the GPU or not at all")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                                # (what is measured so far is kept)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    commit = a.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    commit = commit or "unknown (not a git checkout)"
    say("phase_rate: %s, %s; commit %s" % (torch.cuda.get_device_name(0), m.load_library().mfx_version().decode(), commit))
    k, S, R = 21, 100, 20000
    say("Evaluator.phase at switches %d, range %d; %d runs of each leg, alternating" % (S, R, a.reps))
    # ---- the world
    torch.cuda.set_device(0)
    total = a.mb << 20
    sizes = st.contig_sizes(total, 24)
    truth, layout = st.make_truth(sizes, st.SEED, "cuda:0")
    asm = st.make_assembly(truth, layout, st.SEED)
    del truth
    lens = [int(x.numel()) for x in asm]
    seqs = m.Sequences.from_device([x.data_ptr() for x in asm], lens, device=0)
    ix = m.Index.for_seq(k, total + 1024, device=0)
    ix.claim_seq(seqs)
    n_sets = [0, 0]
    for ci, t in enumerate(asm):
        km, ok = st.canonical_kmers(t, k)
        pos = torch.arange(km.numel(), device=km.device, dtype=torch.int64)
        h = st._hash_range(st.SEED + 9990001 * (ci + 1), 0, km.numel(), km.device)
        pick = ok & ((st._lsr(h, 20) % a.density) == 0)
        hap = ((pos // 50000) & 1) ^ (((pos // 2000) % 37) == 5).to(torch.int64)
        for side in (0, 1):
            sel = km[pick & (hap == side)].contiguous()
            ones = torch.ones(sel.numel(), dtype=torch.int32, device=sel.device)
            (ix.add_read if side == 0 else ix.add_asm)(sel, ones)
            n_sets[side] += int(sel.numel())
        del km, ok, pos, h, pick, hap
    torch.cuda.synchronize()
    info = ix.info()
    ntiles = sum((n + 4095) // 4096 for n in lens)
    say("world: %d Mb synthetic assembly (tools/synth_torch.py), %d contigs, %d tiles, k = %d, sequence-only index (compact = %s); hap-mers drawn from the "
        "assembly at 1 marker in %d positions: %d for A, %d for B" % (a.mb, len(lens), ntiles, k, info.get("compact"), a.density, n_sets[0], n_sets[1]))
    ev = m.Evaluator(ix, m.KParams(26.0))
    # ---- the records agree before anything is timed
    got, cc = ev.phase(seqs, S, R)
    ev.regions(seqs)
    t_dump, t_dump_dev = [], []
    t0 = time.perf_counter()
    want, counts, td = dump_route(pr, ev, seqs, lens, k, S, R)
    t_dump.append(time.perf_counter() - t0)
    t_dump_dev.append(td)
    assert pr.device_records(got) == want, "the device's records differ from the dump route's"
    assert [tuple(int(x) for x in row[1:]) for row in cc] == counts
    say("records of the device path == the dump route's, every field: %d blocks (A %d, B %d), %d markers, %d switch markers; valid k-mers %d, shared %d"
        % (len(got), int((got["hap"] == 0).sum()), int((got["hap"] == 1).sum()), int((got["n_hap"] + got["n_switch"]).sum()), int(got["n_switch"].sum()),
           int(cc[:, 0].sum()), int(cc[:, 3].sum())))
    t_ph, parts, reg_parts = [], [], []
    for rep in range(a.reps):
        ms = []
        t0 = time.perf_counter()
        ev.phase(seqs, S, R, times=ms)
        t_ph.append(time.perf_counter() - t0)
        parts.append(ms)
        ms = []
        ev.regions(seqs, times=ms)
        reg_parts.append(ms)
        if rep + 1 < a.reps:                                     # (the check above was the dump route's first run)
            t0 = time.perf_counter()
            _, _, td = dump_route(pr, ev, seqs, lens, k, S, R)
            t_dump.append(time.perf_counter() - t0)
            t_dump_dev.append(td)
    kasm = int(cc[:, 0].sum())
    rate = lambda s: kasm / s / 1e9
    p, q = np.array(parts), np.array(reg_parts)
    say("phase       : %.2f - %.2f ms (%d runs) = %.3f - %.3f G k-mers/s" % (min(t_ph) * 1e3, max(t_ph) * 1e3, len(t_ph), rate(max(t_ph)), rate(min(t_ph))))
    say("  inside    : pass 1 %.2f - %.2f ms, runs / blocks %.2f - %.2f ms" % (p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max()))
    say("regions     : pass 1 %.2f - %.2f ms on the same index (%d runs)" % (q[:, 0].min(), q[:, 0].max(), len(q)))
    say("dump route  : %.1f - %.1f ms (%d runs), of which mfx_dump_values %.1f - %.1f ms (8 B per position to the host); it does not give the valid k-mers"
        % (min(t_dump) * 1e3, max(t_dump) * 1e3, len(t_dump), min(t_dump_dev) * 1e3, max(t_dump_dev) * 1e3))
    if max(t_ph) < min(t_dump):
        say("  the ranges of phase and of the dump route do not overlap: phase is %.0f - %.0fx faster" % (min(t_dump) / max(t_ph), max(t_dump) / min(t_ph)))
    else:
        say("  the ranges of phase and of the dump route OVERLAP: no speed-up is claimed")
    if p[:, 0].max() < q[:, 0].min():
        say("  pass 1 against regions' pass 1: the ranges do not overlap, phase's takes %.2f - %.2f of its time" % (p[:, 0].min() / q[:, 0].max(), p[:, 0].max() / q[:, 0].min()))
    elif p[:, 0].min() > q[:, 0].max():
        say("  pass 1 against regions' pass 1: the ranges do not overlap, phase's is SLOWER: %.2f - %.2f of its time (not tuned here)"
            % (p[:, 0].min() / q[:, 0].max(), p[:, 0].max() / q[:, 0].min()))
    else:
        say("  pass 1 against regions' pass 1: the ranges overlap")


if __name__ == "__main__":
    main()
