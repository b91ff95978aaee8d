"""The host-side sum of the slots' -hist counts images (csrc/mfx_histsum.h, what every several-slot driver of csrc/mfx_multi.cpp reduces
with) as a stand-alone program under AddressSanitizer + UBSan: tools/native/histsum_sanitize.cpp sizes every image exactly, checks every
sum against one made field by field, and exits non-zero on a mismatch; the sanitizers report on stderr.  No device, no library, nothing
loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_histsum_add_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "histsum_sanitize")
    # (the sanitizers' runtimes linked statically: the program then starts whatever else the environment loads into every process)
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        os.path.join(ROOT, "tools", "native", "histsum_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches)" in r.stdout and "MISMATCH" not in r.stdout
    assert r.stdout.count("\n") >= 2 * 2 * (3 * 6 + 4) + 1          # every case ran
