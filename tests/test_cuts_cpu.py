"""mfx_cut_bins (csrc/mfx_grow.h), the key ranges of the passes of a count, as a stand-alone program under AddressSanitizer + UBSan:
tools/native/cuts_sanitize.cpp cuts bins without entries, one bin, all mass in one bin (first, middle, last), more parts than bins with
entries, counts near 2^64 and 4096 random bins at six values of `parts`, and checks each cutting for "ascending, complete, no range without
entries, largest part minimal" -- on small inputs against every cutting there is.  No device, no library, nothing loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cut_bins_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "cuts_sanitize")
    # (the sanitizers' runtimes linked statically: the program then starts whatever else the environment loads into every process)
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        os.path.join(ROOT, "tools", "native", "cuts_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches" in r.stdout and "MISMATCH" not in r.stdout
    assert r.stdout.count("\n") >= 150                               # every case ran
