"""The host arithmetic of the packed transport of an assembly in host memory -- the streamed -hist and mfx_seq_upload (csrc/mfx_stream.cpp) --
as a stand-alone program under AddressSanitizer + UBSan: tools/native/stream_plan_check.cpp includes csrc/mfx_stream_plan.h, links the encoder
(csrc/mfx_pack.cpp) and checks the chunk cuts (properties, and the literal production schedule for six run lengths), the chunks and their
pieces over hand-made contig layouts, and every host thread's share of a chunk against one mfx_pack_bases call per contig, into buffers
sized exactly.  No device, no library, nothing loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host-only code (csrc/Makefile: mfx_pack.o); it builds this program too"
    exe = str(tmp_path / "stream_plan_check")
    b = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-std=c++17", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "merfin_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                        os.path.join(ROOT, "tools", "native", "stream_plan_check.cpp"), os.path.join(ROOT, "merfin_amd", "csrc", "mfx_pack.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    assert "OK (0 mismatches, 9 cases)" in r.stdout and "MISMATCH" not in r.stdout
