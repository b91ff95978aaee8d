"""Rate of the copy-number spectrum pass (mfx_spectrum_run; mfx_spectrum_kernel) on the device, on the two shapes it meets:

  (a) the full joint table of a --mb Mb synthetic world at load factor 0.7 -- what `merfin -spectrum -readmers` builds: about
      half the entries are read-only error k-mers, most slots are occupied;
  (b) the sequence-only compact k = 21 table of the same world at load factor 0.4 -- what `-hist -peak auto` builds: most
      slots are empty, the single-copy row dominates.

Per shape, in ONE process: the kernel's time between two HIP events (mfx_diag_spectrum_time), plain LDS atomics against the
wave-aggregated form, alternating, --reps passes each after a warm-up; the wall time of Index.spectrum (allocation, clearing,
kernel, copy of the image); and on (a) the wall time of Evaluator.completeness_pieces -- mfx_completeness_kernel streams the same
lines -- on the same table.  Lines per second and bytes per second are the table's 128-byte lines over the kernel time.

    python tools/spectrum_rate.py [--mb 256] [--reps 7] [--shape a|b|ab] [--out profiles/spectrum_pass.txt] [--commit ID]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shape", default="ab")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the tree was built from, where the tree is not a git checkout")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    from tools import synth_torch as st
    if m.device_count() < 1:
        raise SystemExit("spectrum_rate: no HIP device visible; the rate is measured on the GPU or not at all")
    k, lam, copies, mm = 21, 26.0, 4, 10000
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
    say("spectrum_rate: %s, %s; commit %s" % (torch.cuda.get_device_name(0), m.load_library().mfx_version().decode(), commit or "unknown (not a git checkout)"))
    med = lambda v: float(np.median(v))
    for shape in a.shape:
        seq_only = shape == "b"
        os.environ["MFX_LOAD_FACTOR"] = "0.4" if seq_only else "0.7"
        ix, seqs, asm, info = st.build_world(m, a.mb << 20, k=k, lam=lam, ncontigs=24, seq_only=seq_only)
        del os.environ["MFX_LOAD_FACTOR"]
        nlines = info["bytes"] // 128
        say("")
        say("shape (%s): %d Mb synthetic world, k = %d, %s, load factor %s: %d k-mers in %.2f GB (%d lines; the side table included)"
            % (shape, a.mb, k, "sequence-only compact table" if seq_only else "full joint table", "0.4" if seq_only else "0.7", info["distinct"], info["bytes"] / 1e9, nlines))
        img, n = ix.spectrum(copies, mm, with_entries=True)
        pk = m.spectrum_peak(img[1])
        say("  image %d x %d: %d entries; row 0 (read-only) %d, cell (1 copy, 0 reads) %d, largest cell %d = %.1f %% of the entries; peak rule: %s"
            % (copies + 2, mm + 1, n, int(img[0].sum()), int(img[1, 0]), int(img.max()), 100.0 * int(img.max()) / max(n, 1), pk))
        t = {0: [], 1: []}
        for agg in (0, 1):
            ix.spectrum_kernel_ms(copies, mm, bool(agg), 2)          # warm-up
        for rep in range(a.reps):
            for agg in (0, 1):
                t[agg] += ix.spectrum_kernel_ms(copies, mm, bool(agg), 1)
        for agg in (0, 1):
            ms = med(t[agg])
            say("  kernel, %-15s: median %.3f ms (min %.3f, max %.3f; %d passes) = %.2f G lines/s = %.2f TB/s = %.1f %% of the 8 TB/s peak"
                % ("wave-aggregated" if agg else "plain atomics", ms, min(t[agg]), max(t[agg]), len(t[agg]), nlines / ms / 1e6, nlines * 128 / ms / 1e9,
                   100.0 * nlines * 128 / (ms * 1e-3) / HBM_PEAK))
        say("  aggregated / plain: %.3f" % (med(t[1]) / med(t[0])))
        wall = []
        for rep in range(a.reps):
            t0 = time.perf_counter()
            ix.spectrum(copies, mm)
            wall.append(time.perf_counter() - t0)
        say("  Index.spectrum wall (allocation, clearing, kernel, %d KB image to the host): median %.3f ms" % ((copies + 2) * (mm + 1) * 8 // 1024, med(wall) * 1e3))
        t0 = time.perf_counter()
        for rep in range(a.reps):
            m.spectrum_peak(img[1])
        say("  mfx_spectrum_peak on row 1: %.3f ms" % ((time.perf_counter() - t0) / a.reps * 1e3))
        if not seq_only:
            kp = m.KParams.from_file(lam, os.path.join(ROOT, "tests", "golden", "example_lookup_table.txt"))
            ev = m.Evaluator(ix, kp)
            ev.completeness_pieces()
            cw = []
            for rep in range(a.reps):
                t0 = time.perf_counter()
                ev.completeness_pieces()
                cw.append(time.perf_counter() - t0)
            say("  Evaluator.completeness_pieces wall (mfx_completeness_kernel over the same lines + 1 KB to the host): median %.3f ms (min %.3f); "
                "spectrum wall / completeness wall %.3f" % (med(cw) * 1e3, min(cw) * 1e3, med(wall) / med(cw)))
            del ev
        del ix, seqs, asm
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
