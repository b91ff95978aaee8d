"""Seeded read sets for the read k-mer counter (mfx_reads_*, `merfin -reads`): reads sampled from a tests/synth.py truth on
both strands, with substitution errors, N runs, lower-case stretches, reads shorter than k, empty records and reads of
exactly k bases.  Pure numpy; the expected counts come from the oracle's `meryl count` of the same records."""
import numpy as np

from tests import synth

_COMP = bytes.maketrans(b"ACGTacgtNn", b"TGCAtgcaNn")


def revcomp(b):
    return b.translate(_COMP)[::-1]


def sample_reads(r, truth, n_reads, k, lens=(60, 400), sub_rate=0.004, n_run_frac=0.03, lower_frac=0.05):
    """n_reads records (bytes) from the truth contigs (list of bytes), plus the edge cases"""
    truth = [t for t in truth if len(t) >= lens[0]]
    w = np.array([len(t) for t in truth], dtype=np.float64)
    w /= w.sum()
    reads = []
    for _ in range(n_reads):
        t = truth[int(r.choice(len(truth), p=w))]
        L = int(min(len(t), r.integers(lens[0], lens[1] + 1)))
        p = int(r.integers(0, len(t) - L + 1))
        s = bytearray(t[p:p + L])
        for i in np.nonzero(r.random(L) < sub_rate)[0]:
            c = s[i] & 0xDF
            if c in b"ACGT":
                s[i] = b"ACGT"[(b"ACGT".index(c) + int(r.integers(1, 4))) % 4]
        if r.random() < n_run_frac and L > 20:
            q, n = int(r.integers(0, L - 10)), int(r.integers(1, 10))
            s[q:q + n] = b"N" * n
        if r.random() < lower_frac and L > 30:
            q = int(r.integers(0, L - 30))
            s[q:q + 30] = bytes(s[q:q + 30]).lower()
        s = bytes(s)
        reads.append(revcomp(s) if r.random() < 0.5 else s)
    t0 = truth[0]
    reads += [b"", t0[:k - 1], t0[5:5 + k], revcomp(t0[50:50 + k]), b"N" * (3 * k), t0[100:100 + k].lower()]
    order = r.permutation(len(reads))
    return [reads[i] for i in order]


def reads_world(k, seed, sizes=(30000, 9000, 4096, 500), n_reads=3000, lens=(60, 400)):
    """(assembly contigs, reads): the assembly is the truth with errors and decorations (tests/synth.py), the reads are
    sampled from the truth"""
    r = synth.rng(seed)
    truth = synth.make_truth(r, sizes, tandem=(37, 60))
    asm = synth.as_bytes(synth.decorate(r, synth.mutate(r, truth)))
    reads = sample_reads(r, synth.as_bytes(truth), n_reads, k, lens)
    return asm, reads


def low_complexity_reads(r, n_each=400, L=300):
    """reads that send equal keys through one wave: homopolymers, (TTAGGG)n telomere, a 5-mer tandem array, a dinucleotide
    repeat -- enough of them that counts pass 2047 and 65535"""
    out = []
    units = [b"A", b"C", b"TTAGGG", b"CCCTA", b"AC"]
    for u in units:
        rep = (u * (L // len(u) + 2))
        for _ in range(n_each):
            o = int(r.integers(0, len(u)))
            s = rep[o:o + L]
            out.append(revcomp(s) if r.random() < 0.5 else s)
    return out
