"""Rates of `merfin -count`'s device side: the claiming read counter (mfx_reads_begin_all, mfx_reads_kernel<true>), the growths of its table
(mfx_table_rehash_kernel) and the table written as a sorted database (mfx_index_write_db) -- with the update-only counter of `-reads`
(mfx_reads_begin on a sequence-only index of the genome) on the same reads as context, the two alternating in one visit.

A seeded i.i.d. genome of --mb Mb is generated ON THE DEVICE with torch (as tools/reads_count_rate.py does); reads of --len bases at
--cov x, both strands, with substitution errors at --err per base, are sampled on the device and handed to the counter chunk by chunk
straight from host arrays.  Kernel rates are the reads' k-mers over the counter's kernel time (hipEvents around each launch), wall rates
include the host's batching, packing, the copies, and -- the claiming counter -- the growths.

    python tools/count_rate.py [--mb 256] [--cov 30] [--len 150] [--err 0.005] [--k 21] [--reps 2] [--out DIR] [--claim-only]
"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _read_chunk(torch, src, nreads, L, err, g):
    """[nreads, L] ASCII reads of the code tensor `src` with substitutions, odd rows reverse-complemented (on the device)"""
    starts = torch.randint(0, src.numel() - L, (nreads,), generator=g, device="cuda")
    codes = src[starts[:, None] + torch.arange(L, device="cuda")[None, :]]
    if err > 0:
        hit = torch.rand(codes.shape, generator=g, device="cuda") < err
        codes = torch.where(hit, (codes + torch.randint(1, 4, codes.shape, generator=g, device="cuda", dtype=torch.uint8)) & 3, codes)
    rc = (3 - codes).flip(1)                                   # A<->T, C<->G in the order A C G T
    codes[1::2] = rc[1::2]
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    return lut[codes.long()]


def _feed(torch, L, r, world, a, nreads):
    """all reads through mfx_reads_add; (seconds generating, seconds in mfx_reads_add)"""
    g = torch.Generator(device="cuda").manual_seed(7)
    chunk = 1 << 20
    t_gen = t_add = 0.0
    done = 0
    while done < nreads:
        c = min(chunk, nreads - done)
        tg = time.time()
        host = _read_chunk(torch, world, c, a.len, a.err, g).cpu().numpy()
        t_gen += time.time() - tg
        ta = time.time()
        ptrs = (C.c_char_p * c).from_buffer_copy(np.arange(c, dtype=np.uint64) * a.len + host.ctypes.data)
        lens = np.full(c, a.len, dtype=np.uint64)
        rc = L.mfx_reads_add(r, ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)), c)
        assert rc == 0, L.mfx_last_error()
        t_add += time.time() - ta
        done += c
    return t_gen, t_add


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--cov", type=float, default=30.0)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--claim-only", action="store_true", help="only the claiming counter's leg (A/B of two builds through MFX_LIB)")
    ap.add_argument("--out", default=None, help="directory of the database written (default: tmpfs)")
    a = ap.parse_args()
    import torch
    import merfin_amd as m
    from merfin_amd.binding import _ReadsStats
    L = m.load_library()
    n = a.mb << 20
    g0 = torch.Generator(device="cuda").manual_seed(20261018)
    world = torch.randint(0, 4, (n,), generator=g0, device="cuda", dtype=torch.uint8)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    world_ascii = lut[world.long()]
    torch.cuda.synchronize()
    seqs = m.Sequences.from_device([world_ascii.data_ptr()], [n])
    nreads = int(a.cov * n / a.len)
    print("k=%d genome=%d Mb (device-generated, i.i.d.)  reads=%d x %d bases (%.0fx), %.3f %% substitutions" % (a.k, a.mb, nreads, a.len, a.cov, 100 * a.err),
          flush=True)
    out_dir = a.out or tempfile.mkdtemp(prefix="mfx_count_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    db = os.path.join(out_dir, "reads.mfxk")
    try:
        for rep in range(a.reps):
            # ---- the claiming counter into a table created small
            ix = m.Index(a.k, 1024)
            r = L.mfx_reads_begin_all(ix.h, 0)
            assert r, L.mfx_last_error()
            t0 = time.time()
            t_gen, t_add = _feed(torch, L, r, world, a, nreads)
            st = _ReadsStats()
            assert L.mfx_reads_end(r, C.byref(st)) == 0, L.mfx_last_error()
            wall = time.time() - t0
            info, gr = ix.info(), ix.growths()
            print("rep %d  claiming    k-mers %.3f G  distinct %.3f G  kernel %.4f s = %.2f G k-mers/s  copy %.4f s  whole call %.2f s = %.2f G k-mers/s "
                  "(of it: generating the reads %.2f s, mfx_reads_add %.2f s)" % (rep, st.kmers / 1e9, info["distinct"] / 1e9, st.seconds_kernel,
                  st.kmers / max(st.seconds_kernel, 1e-9) / 1e9, st.seconds_copy, wall, st.kmers / max(wall - t_gen, 1e-9) / 1e9, t_gen, t_add), flush=True)
            print("rep %d  growths     %d, %.3f s in all, of it the rehash kernels %.4f s over %.2f GB = %.0f GB/s; final table %.2f GB at load %.3f"
                  % (rep, gr["growths"], gr["seconds"], gr["rehash_seconds"], gr["rehash_bytes"] / 1e9,
                     gr["rehash_bytes"] / 1e9 / max(gr["rehash_seconds"], 1e-9), info["bytes"] / 1e9, info["distinct"] / info["capacity"]), flush=True)
            assert st.dropped == 0 and st.counted == st.kmers
            if a.claim_only:
                ix.close()
                continue
            tw = time.time()
            nk = ix.write_db(db, 0)
            tw = time.time() - tw
            print("rep %d  write_db    %.3f G k-mers in %.2f s = %.1f M k-mers/s, file %.2f GB (%.2f bytes per k-mer)" % (rep, nk / 1e9, tw, nk / tw / 1e6,
                  os.path.getsize(db) / 1e9, os.path.getsize(db) / max(nk, 1)), flush=True)
            assert nk == info["distinct"]
            ix.close()
            os.remove(db)
            # ---- context: the update-only counter of -reads on the k-mers of the genome
            sx = m.Index.for_seq(a.k, n + 16, load_factor=0.4)
            sx.count_asm(seqs)
            torch.cuda.synchronize()
            r = L.mfx_reads_begin(sx.h, 0)
            assert r, L.mfx_last_error()
            t0 = time.time()
            t_gen, t_add = _feed(torch, L, r, world, a, nreads)
            st = _ReadsStats()
            assert L.mfx_reads_end(r, C.byref(st)) == 0, L.mfx_last_error()
            wall = time.time() - t0
            print("rep %d  update-only k-mers %.3f G  counted %.3f G  dropped %.3f G  kernel %.4f s = %.2f G k-mers/s  copy %.4f s  whole call %.2f s = "
                  "%.2f G k-mers/s (of it: generating the reads %.2f s, mfx_reads_add %.2f s)" % (rep, st.kmers / 1e9, st.counted / 1e9, st.dropped / 1e9,
                  st.seconds_kernel, st.kmers / max(st.seconds_kernel, 1e-9) / 1e9, st.seconds_copy, wall, st.kmers / max(wall - t_gen, 1e-9) / 1e9, t_gen, t_add),
                  flush=True)
            sx.close()
    finally:
        if os.path.exists(db):
            os.remove(db)
        if not a.out:
            os.rmdir(out_dir)


if __name__ == "__main__":
    main()
