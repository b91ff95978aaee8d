"""`merfin -reads FILE -k K`: every flag check of the read route fails before any device is touched, with its exact message
(runs on a host without a GPU); the counting itself is checked on the GPU (tests/test_gpu_cli_reads.py)."""
import os

import numpy as np

from tests.test_cli import EXE, _write_text_db, run


def _base(*extra):
    return ["-hist", "-sequence", "asm.fa", "-output", "o", "-peak", "10"] + list(extra)


def test_reads_flag_validation(tmp_path):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    r = run(_base("-reads", "r.fq"))
    assert r.returncode == 1 and "-reads needs -k (or -seqmers, whose k it then takes).\n" in r.stderr
    assert "No read meryl database (-readmers) supplied." not in r.stderr
    for bad in ("0", "65", "x", "21x"):
        r = run(_base("-reads", "r.fq", "-k", bad))
        assert r.returncode == 1 and ("Invalid -k '%s': k is 1 to 64.\n" % bad) in r.stderr
    db = str(tmp_path / "asm.txt")
    _write_text_db(db, 15, np.array([5, 77, 1000], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint32))
    r = run(_base("-reads", "r.fq", "-k", "21", "-seqmers", db))
    assert r.returncode == 1 and "-k 21 disagrees with -seqmers, which holds 15-mers.\n" in r.stderr
    r = run(_base("-reads", "r.fq", "-k", "21", "-readmers", "db"))
    assert r.returncode == 1 and "-reads and -readmers cannot be combined: the read counts come from one source.\n" in r.stderr
    r = run(["-completeness", "-sequence", "a.fa", "-peak", "10", "-reads", "r.fq", "-k", "21"])
    assert r.returncode == 1 and "-completeness needs every read k-mer: it takes a read database (-readmers), not -reads.\n" in r.stderr
    r = run(_base("-reads", "r.fq", "-k", "21", "-sharded", "-devices", "0,1"))
    assert r.returncode == 1 and "-sharded does not take -reads (give the read database with -readmers).\n" in r.stderr
    r = run(["-convert", "db", "-output", "o", "-reads", "r.fq", "-k", "21"])
    assert r.returncode == 1 and "-convert rewrites a k-mer database; it does not take -reads.\n" in r.stderr
    r = run(["-polish", "-sequence", "a.fa", "-vcf", "v.vcf", "-output", "o", "-peak", "10", "-reads", "r.fq", "-k", "33"])
    assert r.returncode == 1 and "The variant modes count -reads into the path-only index, which holds k <= 31 (here k = 33).\n" in r.stderr
    r = run(["-polish", "-sequence", "a.fa", "-vcf", "v.vcf", "-output", "o", "-peak", "10", "-reads", "r.fq", "-k", "21", "-index", "ix"])
    assert r.returncode == 1 and "The variant modes count -reads into the path-only index of the call set: one device, no -index.\n" in r.stderr
    r = run(_base("-reads", str(tmp_path / "missing.fq"), "-k", "21"))
    assert r.returncode == 1 and ("Cannot read the -reads file '%s'.\n" % (tmp_path / "missing.fq")) in r.stderr
    r = run(_base("-readmers", "db", "-k", "21"))
    assert r.returncode == 1 and "-k is taken from -readmers; give -k only with -reads.\n" in r.stderr
    # neither source: the reference's message, unchanged
    r = run(_base())
    assert r.returncode == 1 and "No read meryl database (-readmers) supplied." in r.stderr
    # the usage text names the two flags
    assert "-reads file" in r.stderr and "-k k " in r.stderr
