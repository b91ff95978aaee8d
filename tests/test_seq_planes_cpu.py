"""The bookkeeping behind "a resident sequence gets its packed planes once, or stays one byte per base" (csrc/mfx_internal.h:
mfx_seq_planes_once, what mfx_seq_from_device and the one-byte-per-base mfx_seq_upload call) as a stand-alone program under
AddressSanitizer + UBSan: tools/native/seq_planes_check.cpp supplies the allocator, the release and the fill, fails each of them
in turn, and checks what the sequence object owns and says afterwards.  No device, no library, nothing loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seq_planes_once_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "seq_planes_check")
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "merfin_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                        os.path.join(ROOT, "tools", "native", "seq_planes_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches, 7 cases)" in r.stdout and "MISMATCH" not in r.stdout
