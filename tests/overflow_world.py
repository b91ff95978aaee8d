"""A world whose K* histogram reaches far beyond the dense device image, on both sides and in every part of the tile range: what a
reduction over slots must carry through every slot's overflow list (tests/test_gpu_streamed_multi.py, tests/test_gpu_multi_drivers.py)."""
import numpy as np

from oracle import pyoracle as po
from tests import synth


def overflow_world(tiles):
    """two contigs of `tiles` tiles (the second 11 bases longer); asmK/readK ratios > 13107 (K* bin >= 65536: beyond the default dense
    image) at both ends of both contigs.  Returns k, peak, contigs, read, asm."""
    k = 21
    r = synth.rng(331)
    contigs = [synth.random_contig(r, tiles * 4096).tobytes(), synth.random_contig(r, tiles * 4096 + 11).tobytes()]
    ak, av = po.count_kmers(k, contigs)
    av = av.copy()
    rv = np.full(len(ak), 5, dtype=np.uint32)
    first = po.count_kmers(k, [contigs[0][:60], contigs[0][-60:], contigs[1][:60], contigs[1][-60:]])[0]
    hot = np.isin(ak, first)
    av[hot] = 70000 + (np.arange(hot.sum()) % 7) * 100000     # undr bins 349 995 ... 3.3 M
    rv[np.isin(ak, po.count_kmers(k, [contigs[1][5000:5040]])[0])] = 900000   # over bins ~ 900 000
    return k, 5.0, contigs, (ak, rv), (ak, av)
