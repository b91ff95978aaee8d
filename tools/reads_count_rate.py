"""Rate of the read k-mer counter (mfx_reads_*, mfx_reads_kernel) on the device, and the phases of `merfin -hist -reads`.

Kernel leg: a seeded i.i.d. world of --mb Mb is generated ON THE DEVICE with torch and claimed on a sequence-only index (k = 21, the
CLI's load factor 0.4).  Reads of --len bases at --cov x, both strands, are sampled on the device as well and handed to the counter
chunk by chunk straight from host arrays (no parsing, no Python objects per read): once i.i.d., once as a low-complexity-heavy set
(half the reads from homopolymer / (TTAGGG)n / 5-mer arrays).  The kernel rate is the reads' k-mers over the counter's kernel time
(hipEvents around each launch: resident batches); the wall rate includes the host's batching, packing and the copies.

CLI leg (--cli MB): the reads of an MB Mb world at --cov x written as FASTQ, plain in tmpfs (/dev/shm) and gzip'ed, then
`merfin -hist -reads ... -k 21` with MFX_CLI_TIMING=2: the counter's wall, the time spent waiting for parsed records, the time in
mfx_reads_add (batching, encoding, waiting for a stage), the device's kernel and copy time and its idle share.

    python tools/reads_count_rate.py [--mb 256] [--cov 20] [--len 150] [--cli 16]
"""
import argparse
import ctypes as C
import gzip
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)


def _world(torch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 4, (n,), generator=g, device="cuda", dtype=torch.uint8)        # codes 0..3 = A C G T


def _read_chunk(torch, src, nreads, L, g):
    """[nreads, L] ASCII reads of the code tensor `src`, odd rows reverse-complemented (on the device)"""
    starts = torch.randint(0, src.numel() - L, (nreads,), generator=g, device="cuda")
    codes = src[starts[:, None] + torch.arange(L, device="cuda")[None, :]]
    rc = (3 - codes).flip(1)                                   # A<->T, C<->G in the order A C G T
    codes[1::2] = rc[1::2]
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    return lut[codes.long()]


def kernel_leg(a):
    import torch
    import merfin_amd as m
    L = m.load_library()
    n = a.mb << 20
    world = _world(torch, n, 20261016)
    low = torch.tensor(list(b"A" * 4000 + b"TTAGGG" * 700 + b"CCCTA" * 800 + b"C" * 4000), dtype=torch.uint8, device="cuda")
    low_codes = ((low >> 1) & 3)                                # A 0 C 1 T 2 G 3 ...
    low_codes = torch.where(low_codes == 2, 3, torch.where(low_codes == 3, 2, low_codes)).to(torch.uint8)   # ... as A C G T codes
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    world_ascii = lut[world.long()]
    torch.cuda.synchronize()
    seqs = m.Sequences.from_device([world_ascii.data_ptr(), low.data_ptr()], [n, low.numel()])
    nreads = int(a.cov * n / a.len)
    chunk = 1 << 20
    print("k=%d world=%d Mb (device-generated)  reads=%d x %d bases (%.0fx), %d reads per chunk" % (a.k, a.mb, nreads, a.len, a.cov, chunk), flush=True)
    for name, frac_low in (("iid", 0.0), ("low-complexity 50%", 0.5)):
        ix = m.Index.for_seq(a.k, n + low.numel() + 16, load_factor=0.4)
        ix.count_asm(seqs)
        torch.cuda.synchronize()
        g = torch.Generator(device="cuda").manual_seed(7)
        r = L.mfx_reads_begin(ix.h, 0)
        assert r, L.mfx_last_error()
        t_gen = t_add = 0.0
        t0 = time.time()
        done = 0
        while done < nreads:
            c = min(chunk, nreads - done)
            tg = time.time()
            nl = int(c * frac_low)
            parts = []
            if c - nl:
                parts.append(_read_chunk(torch, world, c - nl, a.len, g))
            if nl:
                parts.append(_read_chunk(torch, low_codes.repeat(4), nl, a.len, g))
            host = torch.cat(parts).cpu().numpy()
            t_gen += time.time() - tg
            ta = time.time()
            base = host.ctypes.data
            ptrs = (C.c_char_p * c).from_buffer_copy(np.arange(c, dtype=np.uint64) * a.len + base)
            lens = np.full(c, a.len, dtype=np.uint64)
            rc = L.mfx_reads_add(r, ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)), c)
            assert rc == 0, L.mfx_last_error()
            t_add += time.time() - ta
            done += c
        from merfin_amd.binding import _ReadsStats
        st = _ReadsStats()
        assert L.mfx_reads_end(r, C.byref(st)) == 0, L.mfx_last_error()
        wall = time.time() - t0
        print("%-20s kmers %.3f G  counted %.3f G  dropped %.3f G  side %d  kernel %.4f s = %.1f G k-mers/s  copy %.4f s  "
              "host: generate %.2f s, mfx_reads_add %.2f s (batching + packing, %.2f G k-mers/s)"
              % (name, st.kmers / 1e9, st.counted / 1e9, st.dropped / 1e9, st.saturated, st.seconds_kernel, st.kmers / max(st.seconds_kernel, 1e-9) / 1e9,
                 st.seconds_copy, t_gen, t_add, st.kmers / max(t_add, 1e-9) / 1e9), flush=True)
        ix.close()


def cli_leg(a):
    import torch
    n = a.cli << 20
    world = _world(torch, n, 99)
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else None
    d = tempfile.mkdtemp(prefix="mfx_reads_cli_", dir=tmp)
    try:
        fa = os.path.join(d, "asm.fa")
        with open(fa, "wb") as f:
            f.write(b">asm\n" + ASCII[world.cpu().numpy()].tobytes() + b"\n")
        fq = os.path.join(d, "reads.fq")
        g = torch.Generator(device="cuda").manual_seed(5)
        nreads = int(a.cov * n / a.len)
        with open(fq, "wb") as f:
            for o in range(0, nreads, 1 << 20):
                c = min(1 << 20, nreads - o)
                rd = _read_chunk(torch, world, c, a.len, g).cpu().numpy()
                rows = np.empty((c, 2 * a.len + 7), dtype=np.uint8)
                rows[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
                rows[:, 3:3 + a.len] = rd
                rows[:, 3 + a.len:6 + a.len] = np.frombuffer(b"\n+\n", dtype=np.uint8)
                rows[:, 6 + a.len:6 + 2 * a.len] = ord("I")
                rows[:, -1] = ord("\n")
                f.write(rows.tobytes())
        gz = fq + ".gz"
        with open(fq, "rb") as fi, gzip.open(gz, "wb", compresslevel=1) as fo:
            shutil.copyfileobj(fi, fo, 1 << 24)
        exe = os.path.join(ROOT, "merfin_amd", "bin", "merfin")
        print("CLI: world %d Mb, %d reads x %d bases (%.0fx): FASTQ %.2f GB in %s, gz %.2f GB" % (a.cli, nreads, a.len, a.cov, os.path.getsize(fq) / 1e9,
              tmp or "tmp", os.path.getsize(gz) / 1e9), flush=True)
        for name, path in (("plain FASTQ", fq), ("gz FASTQ", gz)):
            env = dict(os.environ, MFX_CLI_TIMING="2")
            t = time.time()
            p = subprocess.run([exe, "-hist", "-sequence", fa, "-reads", path, "-k", str(a.k), "-peak", "20", "-output", os.path.join(d, "h")],
                               capture_output=True, text=True, env=env)
            wall = time.time() - t
            assert p.returncode == 0, p.stderr
            print("%s: process wall %.2f s" % (name, wall))
            for line in p.stderr.splitlines():
                if line.startswith("-- reads:") or line.startswith("-- Counted") or "timing" in line.lower() or line.startswith("--   "):
                    print("  " + line)
            sys.stdout.flush()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--cov", type=float, default=20.0)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--cli", type=int, default=0, help="world size (Mb) of the CLI leg; 0: no CLI leg")
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    if not a.no_kernel:
        kernel_leg(a)
    if a.cli:
        cli_leg(a)


if __name__ == "__main__":
    main()
