"""The device arena of a batch of the variant modes (csrc/mfx_var_arena.h: what mfx_score_paths, mfx_score_paths_trv and
mfx_claim_paths_batch carve out of one allocation) as a stand-alone program under AddressSanitizer + UBSan: tools/native/var_arena_check.cpp
lays every shape out over a host block of exactly the bytes the layout asks for -- an empty batch, a host part, a device part, both, no rows,
need_dk 0 and 1, the claim form with and without a batch, each at text lengths 0, 1, 4095, 4096 and 4097 -- and checks the 256-byte
boundaries, that no two pieces overlap, that each holds its array, and the total against the sums the two callers computed before the layout
was shared, written out literally.  No device, no library, nothing loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_var_arena_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "var_arena_check")
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "merfin_amd", "csrc"), os.path.join(ROOT, "tools", "native", "var_arena_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches, 18 cases)" in r.stdout and "MISMATCH" not in r.stdout
