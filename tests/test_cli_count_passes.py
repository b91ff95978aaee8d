"""`merfin -count -passes P|auto`: every mistake in -passes is refused with return code 1 and its own sentence before any device is touched
(runs on a host without a GPU), and nothing is written; the passes themselves are checked on the GPU (tests/test_gpu_cli_count_passes.py)."""
import os

import pytest

from tests.test_cli import EXE, run


@pytest.fixture()
def reads(tmp_path):
    p = tmp_path / "reads.fasta"
    p.write_bytes(b">r0\nACGTACGTTTGACCAGTTACGGATCAGGACTTTACGAC\n")
    return str(p)


def _refused(args, msg, out):
    r = run(args)
    assert r.returncode == 1 and msg in r.stderr, (args, r.stderr[-900:])
    assert "usage:" in r.stderr and "ERROR: HIP device" not in r.stderr and "-- Counting" not in r.stderr       # no device was opened
    assert not os.path.exists(out)
    return r


def test_passes_refusals(reads, tmp_path):
    assert os.path.exists(EXE), "build the CLI with `make -C merfin_amd/cli`"
    out = str(tmp_path / "reads.mfxk")
    ok = ["-count", "-reads", reads, "-k", "21", "-output", out]
    sentences = {
        "0": "Invalid -passes '0': -count takes at least one pass (1 to 4096, or auto).\n",
        "-1": "Invalid -passes '-1': -count takes at least one pass (1 to 4096, or auto).\n",
        "x": "Invalid -passes 'x': the passes of -count are a number from 1 to 4096, or auto.\n",
        "4097": "Invalid -passes '4097': a pass takes at least one of the 4096 key bins, so there are 4096 at most (or auto).\n",
    }
    for v, msg in sentences.items():
        r = _refused(ok + ["-passes", v], msg, out)
        errs = r.stderr.split("[-comb N (15)] [-nosplit] [-debug -> <output>.00.debug.gz]\n\n", 1)[1]
        assert errs == msg, errs                                    # one mistake, one sentence
    for v in ("3x", "", "1.5", "Auto"):
        _refused(ok + ["-passes", v], "Invalid -passes '%s': the passes of -count are a number from 1 to 4096, or auto.\n" % v, out)
    # -passes belongs to -count
    for v in ("2", "auto"):
        r = _refused(["-hist", "-reads", reads, "-k", "21", "-output", out, "-passes", v],
                     "-passes divides the work of -count: it has no meaning without -count.\n", out)
        assert r.stderr.count("-passes divides the work of -count") == 1


def test_legal_passes_pass_validation(reads, tmp_path):
    """1, 4096 and auto are taken: such a line stops at the device that is not there, or runs"""
    for v in ("1", "4096", "auto"):
        out = str(tmp_path / ("reads_%s.mfxk" % v))
        r = run(["-count", "-reads", reads, "-k", "21", "-output", out, "-passes", v])
        assert "usage:" not in r.stderr and "Invalid -passes" not in r.stderr, r.stderr[-600:]
        assert r.returncode == 0 or "ERROR: HIP device 0 not available" in r.stderr


def test_usage_names_passes():
    r = run([])
    assert r.returncode == 1
    assert "    -passes P|auto    with -count: the k-mers are counted in P passes (1 to 4096) over ascending key ranges" in r.stderr
    assert "    -count            no report: count every k-mer of the -reads files on the GPU" in r.stderr
