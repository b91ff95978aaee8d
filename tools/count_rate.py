"""Rates of `merfin -count`'s device side: the claiming read counter (mfx_reads_begin_all, mfx_reads_kernel<true>), the growths of its table
(mfx_table_rehash_kernel) and the table written as a sorted database (mfx_index_write_db) -- with the update-only counter of `-reads`
(mfx_reads_begin on a sequence-only index of the genome) on the same reads as context, the two alternating in one visit.

A seeded i.i.d. genome of --mb Mb is generated ON THE DEVICE with torch (as tools/reads_count_rate.py does); reads of --len bases at
--cov x, both strands, with substitution errors at --err per base, are sampled on the device and handed to the counter chunk by chunk
straight from host arrays.  Kernel rates are the reads' k-mers over the counter's kernel time (hipEvents around each launch), wall rates
include the host's batching, packing, the copies, and -- the claiming counter -- the growths.

    python tools/count_rate.py [--mb 256] [--cov 30] [--len 150] [--err 0.005] [--k 21] [--reps 2] [--out DIR] [--claim-only]

--passes 1,2,4 [--max-gb G] adds the legs of a count in passes (mfx_reads_begin_range): the same reads are packed once into a read store
(mfx_reads_store_*), then counted from it in P passes over P equal key ranges (NOT equal shares: a canonical k-mer is the smaller of two, so
the quarters of the key space hold 7/16, 5/16, 3/16 and 1/16 of an i.i.d. genome's k-mers -- the CLI cuts by the key histogram instead), each
into an index created small; per pass the kernel seconds, per P the whole call with the writer that joins the tables (DbWriter).
--passes-files adds, at the largest P, passes that take the reads from mfx_reads_add again (generated anew: what a pass from the files pays on
the host).
--max-gb G runs the driver of `-passes auto` under that limit: one range, a refused range cut in two at the median of its table's bins.

--writers adds the leg of the two database writers: the claiming counter's table is written three times with each, alternating (host:
mfx_db_writer_open, the k-mers collected and coded on the host; stream: mfx_db_writer_open_streamed, coded on the device and spooled),
file in tmpfs; the rates, the host memory each held (mfx_db_writer_info) and the MFX_DB_TIMING split of every write are appended to
--profile (default profiles/count_stream.txt).  --writers-only skips the other legs.
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


def _fill_store(torch, m, world, a, nreads):
    """all reads into a read store; (store, seconds generating, seconds in mfx_reads_store_add)"""
    L = m.load_library()
    s = m.ReadsStore(a.k, 0, 0)
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
        assert L.mfx_reads_store_add(s.h, ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)), c) == 0, L.mfx_last_error()
        t_add += time.time() - ta
        done += c
    return s, t_gen, t_add


def _pass_legs(torch, m, world, a, nreads, db):
    """the legs of --passes / --passes-files / --max-gb"""
    from merfin_amd.binding import _ReadsStats
    L = m.load_library()
    top = 4 ** a.k
    store, t_gen, t_add = _fill_store(torch, m, world, a, nreads)
    si = store.info()
    print("store       %d batches, %.2f GB (%.3f bytes per base), filled in %.2f s of mfx_reads_store_add (generating the reads %.2f s)"
          % (si["batches"], si["bytes"] / 1e9, si["bytes"] / max(si["bases"], 1), t_add, t_gen), flush=True)
    for rep in range(a.reps):
        plist = [int(x) for x in a.passes.split(",") if x]
        for P in plist:
            for source in (["store"] + (["add"] if a.passes_files and P > 1 and P == max(plist) else [])):
                w = m.DbWriter(db, a.k)
                t0 = time.time()
                kern, gen_all, n_all = [], 0.0, 0
                for i in range(P):
                    lo, hi = top * i // P, top * (i + 1) // P
                    ix = m.Index(a.k, 1024)
                    tp = time.time()
                    if source == "store":
                        st = store.replay(ix, key_range=(lo, hi))
                        st_k, st_c = st["seconds_kernel"], st["counted"]
                    else:
                        r = L.mfx_reads_begin_range(ix.h, 0, lo, hi)
                        assert r, L.mfx_last_error()
                        tg, _ = _feed(torch, L, r, world, a, nreads)
                        gen_all += tg
                        rs = _ReadsStats()
                        assert L.mfx_reads_end(r, C.byref(rs)) == 0, L.mfx_last_error()
                        st_k, st_c = rs.seconds_kernel, rs.counted
                    tp = time.time() - tp
                    kern.append(st_k)
                    n_all += st_c
                    gr = ix.growths()
                    print("rep %d  P=%d %-5s pass %d  counted %.3f G  distinct %.3f G  kernel %.4f s  pass %.2f s  growths %d (%.3f s)  table %.2f GB"
                          % (rep, P, source, i + 1, st_c / 1e9, ix.info()["distinct"] / 1e9, st_k, tp, gr["growths"], gr["seconds"], ix.info()["bytes"] / 1e9), flush=True)
                    w.append(ix)
                    ix.close()
                t_count = time.time() - t0 - gen_all
                tw = time.time()
                nk = w.close()
                tw = time.time() - tw
                print("rep %d  P=%d %-5s kernels %.4f s in all (%s); counting and collecting %.2f s (the reads' generation taken out), writing %.2f s; %.3f G k-mers counted, "
                      "%.3f G written" % (rep, P, source, sum(kern), " + ".join("%.4f" % x for x in kern), t_count, tw, n_all / 1e9, nk / 1e9), flush=True)
                os.remove(db)
    if a.max_gb > 0:
        # the driver of `-passes auto`: one range; a range whose table cannot grow is cut in two at the median of the bins it reached
        todo, npass, nref = [(0, 4096)], 0, 0
        shift = 2 * a.k - 12
        w = m.DbWriter(db, a.k)
        t0 = time.time()
        while todo:
            blo, bhi = todo.pop(0)
            ix = m.Index(a.k, 1024, max_gb=a.max_gb)
            tp = time.time()
            try:
                st = store.replay(ix, key_range=(blo << shift, bhi << shift))
            except m.MfxError as e:
                assert e.code == -2 and bhi - blo > 1, str(e)
                c = np.cumsum(ix.key_bins(0)[blo:bhi].astype(np.float64))
                cut = blo + 1 + int(np.searchsorted(c[:-1], c[-1] / 2))
                cut = min(max(cut, blo + 1), bhi - 1)
                print("forced      bins [%d, %d) refused after %.2f s at %.2f GB: %s; cut at %d" % (blo, bhi, time.time() - tp, ix.info()["bytes"] / 1e9, str(e)[:110], cut),
                      flush=True)
                ix.close()
                todo[:0] = [(blo, cut), (cut, bhi)]
                nref += 1
                continue
            npass += 1
            print("forced      pass %d bins [%d, %d)  counted %.3f G  distinct %.3f G  kernel %.4f s  pass %.2f s  table %.2f GB"
                  % (npass, blo, bhi, st["counted"] / 1e9, ix.info()["distinct"] / 1e9, st["seconds_kernel"], time.time() - tp, ix.info()["bytes"] / 1e9), flush=True)
            w.append(ix)
            ix.close()
        nk = w.close()
        print("forced      max_gb %.3f: %d passes, %d refused and split, %.3f G k-mers written, %.2f s in all" % (a.max_gb, npass, nref, nk / 1e9, time.time() - t0), flush=True)
        os.remove(db)
    store.close()


def _with_stderr(fn):
    """fn() with the process's stderr (the library's MFX_DB_TIMING lines) caught; (result, text)"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as t:
        os.dup2(t.fileno(), 2)
        try:
            res = fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        t.seek(0)
        return res, t.read().decode(errors="replace")


def _writer_leg(torch, m, L, world, a, nreads, db):
    """the same table through both writers, alternating; the lines go to stdout and to a.profile"""
    import filecmp
    from merfin_amd.binding import _ReadsStats
    ix = m.Index(a.k, 1024)
    r = L.mfx_reads_begin_all(ix.h, 0)
    assert r, L.mfx_last_error()
    _feed(torch, L, r, world, a, nreads)
    st = _ReadsStats()
    assert L.mfx_reads_end(r, C.byref(st)) == 0, L.mfx_last_error()
    info = ix.info()
    lines = ["k=%d genome=%d Mb reads=%d x %d bases (%.0fx): %.3f G k-mers, %.3f G distinct, table %.2f GB; file in %s"
             % (a.k, a.mb, nreads, a.len, a.cov, st.kmers / 1e9, info["distinct"] / 1e9, info["bytes"] / 1e9, os.path.dirname(db))]
    print(lines[0], flush=True)
    os.environ["MFX_DB_TIMING"] = "1"
    other = db + ".other"
    secs = {"host": [], "stream": []}
    try:
        for rep in range(3):
            for kind in ("host", "stream"):
                path = other if (rep == 0 and kind == "stream") else db

                def write():
                    t0 = time.time()
                    w = m.DbWriter(path, a.k, streamed=(kind == "stream"))
                    w.append(ix)
                    held = w.info()
                    return w.close(), held, time.time() - t0
                (nk, held, tw), err = _with_stderr(write)
                assert nk == info["distinct"]
                secs[kind].append(tw)
                size = os.path.getsize(path)
                line = ("rep %d  %-6s %.3f G k-mers in %.2f s = %.1f M k-mers/s, file %.2f GB (%.2f bytes per k-mer); the writer held %.3f GB on the host "
                        "before close (%d blocks in a spool of %.2f GB, %d escapes)"
                        % (rep, kind, nk / 1e9, tw, nk / tw / 1e6, size / 1e9, size / max(nk, 1), held["held_bytes"] / 1e9, held["blocks"],
                           held["spool_bytes"] / 1e9, held["escapes"]))
                print(line, flush=True)
                lines.append(line)
                for x in err.splitlines():
                    if x.startswith("[mfx db]"):
                        print("        " + x, flush=True)
                        lines.append("        " + x)
                if rep == 0 and kind == "stream":
                    same = filecmp.cmp(db, other, shallow=False)
                    line = "rep 0  the two files are %s" % ("equal, byte for byte" if same else "DIFFERENT")
                    print(line, flush=True)
                    lines.append(line)
                    os.remove(other)
                    assert same
        lines.append("host   %s s; stream %s s" % (", ".join("%.2f" % x for x in secs["host"]), ", ".join("%.2f" % x for x in secs["stream"])))
        print(lines[-1], flush=True)
    finally:
        for x in (db, other):
            if os.path.exists(x):
                os.remove(x)
        os.makedirs(os.path.dirname(os.path.abspath(a.profile)), exist_ok=True)
        with open(a.profile, "a") as f:
            f.write("\n".join(lines) + "\n")
    ix.close()


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
    ap.add_argument("--passes", default="", help="e.g. 1,2,4: also count from a read store in that many passes over equal key ranges")
    ap.add_argument("--passes-files", action="store_true", help="with --passes: at the largest P also passes fed through mfx_reads_add again")
    ap.add_argument("--passes-only", action="store_true", help="only the legs of --passes / --max-gb")
    ap.add_argument("--max-gb", type=float, default=0.0, help="with --passes: also the driver of -passes auto under this table limit")
    ap.add_argument("--writers", action="store_true", help="also the leg of the two database writers, three writes each, alternating")
    ap.add_argument("--writers-only", action="store_true", help="only that leg")
    ap.add_argument("--profile", default=os.path.join(ROOT, "profiles", "count_stream.txt"), help="the file --writers appends its lines to")
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
        if a.writers or a.writers_only:
            _writer_leg(torch, m, L, world, a, nreads, db)
        if (a.passes or a.max_gb > 0) and not a.writers_only:
            _pass_legs(torch, m, world, a, nreads, db)
        for rep in range(0 if a.passes_only or a.writers_only else a.reps):
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
