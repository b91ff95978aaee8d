"""The plain host arithmetic of the claiming read counter's table and of mfx_index_write_db's key ranges (csrc/mfx_grow.h) as a stand-alone
program under AddressSanitizer + UBSan: tools/native/grow_sanitize.cpp checks the 0.7 and 0.35 bounds around their edges and the grouping
of bins into ranges (empty bins, a bin larger than a range, the last range) against definitions written out the slow way.  No device, no
library, nothing loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_growth_rule_and_key_ranges_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "grow_sanitize")
    # (the sanitizers' runtimes linked statically: the program then starts whatever else the environment loads into every process)
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        os.path.join(ROOT, "tools", "native", "grow_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches" in r.stdout and "MISMATCH" not in r.stdout
    assert r.stdout.count("\n") >= 150                               # every case ran
