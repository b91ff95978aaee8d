"""Rate of `-bin` (Evaluator.bin_reads / mfx_bin_*: per-read hap-mer counts reduced on the device) against the only route to the same
numbers before it: the same reads joined by `N` into contigs, mfx_dump_values over them (8 bytes per base over the link), then
numpy.add.reduceat per read on the host; and its kernel beside pass 1 of `-phase` (mfx_diag_phase_times) on the same table.

The read set of tools/count_rate.py: a seeded i.i.d. genome of --mb Mb generated on the device, reads of --len bases at --cov x, both
strands, substitutions at --err per base, k = 21.  The table is the full table of two hap-mer sets, each 1 % of the genome's k-mers
drawn by a hash (a placeholder density: no real trio was at hand).  In ONE process, alternating the legs --reps times after the
counts of one chunk were compared:
  bin         : the whole call -- mfx_bin_add chunk by chunk (cutting, packing, copies, kernel, the records' way back), take, end --
                without the time the reads take to generate; beside it the kernel seconds the library timed (hipEvents around each launch);
  dump route  : per chunk of reads one contig (reads joined by N) uploaded, Evaluator.dump_values, three numpy.add.reduceat.  It
                does not give a read's valid k-mers.
No bar is set on a rate: where two ranges overlap the tool says so.

    python tools/bin_rate.py [--mb 256] [--cov 30] [--len 150] [--err 0.005] [--reps 5] [--out profiles/bin_rate.txt] [--commit ID]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 1 << 20          # reads per chunk


def chunks(torch, cr, world, a, nreads):
    """the read set chunk by chunk as host arrays [c, len]; the generator is seeded: every pass sees the same reads"""
    g = torch.Generator(device="cuda").manual_seed(7)
    done = 0
    while done < nreads:
        c = min(CHUNK, nreads - done)
        yield cr._read_chunk(torch, world, c, a.len, a.err, g).cpu().numpy()
        done += c


def bin_leg(torch, m, cr, ev, world, a, nreads, first_only=False):
    """(rows of the first chunk, seconds of the whole call without generating, kernel seconds, seconds in mfx_bin_add, k-mers)"""
    L = m.load_library()
    b = m.Binner(ev, 0)
    t_call = t_add = 0.0
    first = None
    rows = 0
    gen = chunks(torch, cr, world, a, nreads)
    for host in gen:
        c = host.shape[0]
        t0 = time.perf_counter()
        ptrs = (C.c_char_p * c).from_buffer_copy(np.arange(c, dtype=np.uint64) * a.len + host.ctypes.data)
        lens = np.full(c, a.len, dtype=np.uint64)
        rc = L.mfx_bin_add(b.h, ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)), c)
        assert rc == 0, L.mfx_last_error()
        t_add += time.perf_counter() - t0
        got = b.take(b.ready())
        rows += len(got)
        t_call += time.perf_counter() - t0
        if first is None:
            first = [got]
        elif sum(len(x) for x in first) < CHUNK:
            first.append(got)
        if first_only:
            break
    gen.close()
    t0 = time.perf_counter()
    b.flush()
    got = b.take(b.ready())
    rows += len(got)
    if sum(len(x) for x in first) < CHUNK:
        first.append(got)
    st = b.end()
    t_call += time.perf_counter() - t0
    assert rows == st["reads"]
    return np.concatenate(first)[:CHUNK], t_call, st["seconds_kernel"], t_add, st["kmers"]


def dump_leg(torch, m, cr, ev, world, a, nreads, first_only=False):
    """(A only, B only, shared per read of the first chunk; seconds without generating; of it seconds in upload + mfx_dump_values)"""
    t_all = t_dev = 0.0
    first = None
    gen = chunks(torch, cr, world, a, nreads)
    for host in gen:
        c = host.shape[0]
        t0 = time.perf_counter()
        joined = np.full((c, a.len + 1), ord("N"), dtype=np.uint8)
        joined[:, :a.len] = host
        seqs = m.Sequences([joined.tobytes()])
        rv, av, _, _ = ev.dump_values(seqs, 0, 0, joined.size)
        seqs.close()
        t_dev += time.perf_counter() - t0
        starts = np.arange(c, dtype=np.int64) * (a.len + 1)
        ina, inb = rv != 0, av != 0
        cols = [np.add.reduceat((x).astype(np.uint32), starts) for x in (ina & ~inb, inb & ~ina, ina & inb)]
        t_all += time.perf_counter() - t0
        if first is None:
            first = np.stack(cols, axis=1)
        if first_only:
            break
    gen.close()
    return first, t_all, t_dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--cov", type=float, default=30.0)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the tree was built from, where the tree is not a git checkout")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    from tools import count_rate as cr
    from tools import synth_torch as st
    if m.device_count() < 1:
        raise SystemExit("bin_rate: no HIP device visible; the rate is measured on the GPU or not at all")
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
    say("bin_rate: %s, %s; commit %s" % (torch.cuda.get_device_name(0), m.load_library().mfx_version().decode(), commit))
    k = 21
    n = a.mb << 20
    g0 = torch.Generator(device="cuda").manual_seed(20261018)
    world = torch.randint(0, 4, (n,), generator=g0, device="cuda", dtype=torch.uint8)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    world_ascii = lut[world.long()]
    nreads = int(a.cov * n / a.len)
    # ---- the table: two hap-mer sets, 1 % of the genome's k-mers each
    km, ok = st.canonical_kmers(world_ascii, k)
    h = st._lsr(st._hash_range(st.SEED + 4242, 0, km.numel(), km.device), 20) % 100
    sets = [torch.unique(km[ok & (h == side)]) for side in (0, 1)]
    del km, ok, h
    ix = m.Index(k, int(sets[0].numel() + sets[1].numel()) + 1024)
    for side, s in enumerate(sets):
        (ix.add_read if side == 0 else ix.add_asm)(s.contiguous(), torch.ones(s.numel(), dtype=torch.int32, device=s.device))
    torch.cuda.synchronize()
    say("world: %d Mb i.i.d. genome (device-generated), %d reads x %d bases (%.0fx), %.3f %% substitutions, k = %d; full table of two hap-mer sets drawn from the genome's "
        "k-mers at 1 in 100 each (a placeholder density): %d for A, %d for B" % (a.mb, nreads, a.len, a.cov, 100 * a.err, k, sets[0].numel(), sets[1].numel()))
    del sets
    ev = m.Evaluator(ix, m.KParams(1.0))
    # ---- the counts agree before anything is timed (the first chunk of reads)
    rows, _, _, _, _ = bin_leg(torch, m, cr, ev, world, a, nreads, first_only=True)
    cols, _, _ = dump_leg(torch, m, cr, ev, world, a, nreads, first_only=True)
    assert len(rows) == len(cols) and np.array_equal(rows[:, 1:], cols), "the device's counts differ from the dump route's"
    assert (rows[:, 0] == a.len - k + 1).all()
    say("counts of the device path == the dump route's over the first %d reads: A only %d, B only %d, shared %d" % (len(rows), int(rows[:, 1].sum()), int(rows[:, 2].sum()),
                                                                                                            int(rows[:, 3].sum())))
    # ---- pass 1 of -phase on the same table, over the genome
    seqs = m.Sequences.from_device([world_ascii.data_ptr()], [n])
    t_bin, t_kern, t_add, t_dump, t_dump_dev, ph = [], [], [], [], [], []
    kmers = 0
    for rep in range(a.reps):
        _, tc, tk, ta, kmers = bin_leg(torch, m, cr, ev, world, a, nreads)
        t_bin.append(tc); t_kern.append(tk); t_add.append(ta)
        ms = []
        _, cc = ev.phase(seqs, times=ms)
        ph.append(int(cc[:, 0].sum()) / (ms[0] * 1e-3) / 1e9)
        _, td, tv = dump_leg(torch, m, cr, ev, world, a, nreads)
        t_dump.append(td); t_dump_dev.append(tv)
        print("run %d: bin %.2f s (kernel %.3f s), dump route %.2f s" % (rep, tc, tk, td), flush=True)
    rate =lambda s: kmers / s / 1e9
    say("bin         : %.2f - %.2f s the whole call (%d runs, %.3f G k-mers) = %.3f - %.3f G k-mers/s" % (min(t_bin), max(t_bin), len(t_bin), kmers / 1e9, rate(max(t_bin)),
                                                                                                        rate(min(t_bin))))
    say("  kernel    : %.3f - %.3f s = %.2f - %.2f G k-mers/s; pass 1 of -phase on the same table over the genome: %.2f - %.2f G k-mers/s" % (
        min(t_kern), max(t_kern), rate(max(t_kern)), rate(min(t_kern)), min(ph), max(ph)))
    say("  host      : %.2f - %.2f s of the whole call are spent inside mfx_bin_add (cutting, packing, waiting for a stage): %.0f - %.0f %% of it" % (
        min(t_add), max(t_add), 100 * min(x / y for x, y in zip(t_add, t_bin)), 100 * max(x / y for x, y in zip(t_add, t_bin))))
    say("dump route  : %.2f - %.2f s (%d runs), of which upload + mfx_dump_values %.2f - %.2f s (8 B per base to the host)" % (min(t_dump), max(t_dump), len(t_dump),
                                                                                                                       min(t_dump_dev), max(t_dump_dev)))
    if max(t_bin) < min(t_dump):
        say("  the ranges of bin and of the dump route do not overlap: bin is %.1f - %.1fx faster" % (min(t_dump) / max(t_bin), max(t_dump) / min(t_bin)))
    else:
        say("  the ranges of bin and of the dump route OVERLAP: no speed-up is claimed")
    kr = (rate(max(t_kern)), rate(min(t_kern)))
    if kr[1] < min(ph):
        say("  the kernel against pass 1 of -phase: the ranges do not overlap, bin's is SLOWER: %.2f - %.2f of its rate (not tuned here)" % (kr[0] / max(ph), kr[1] / min(ph)))
    elif kr[0] > max(ph):
        say("  the kernel against pass 1 of -phase: the ranges do not overlap, bin's is faster: %.2f - %.2f of its rate" % (kr[0] / max(ph), kr[1] / min(ph)))
    else:
        say("  the kernel against pass 1 of -phase: the ranges overlap")


if __name__ == "__main__":
    main()
