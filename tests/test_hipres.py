"""CPU tier: the owning HIP handles of rtlsdrdiags_amd/csrc/iqd_hipres.h, instantiated with a counting fake release function
and a malloc-backed fake allocator (tests/hipres/hipres_check.cpp: a stand-alone program, built here with AddressSanitizer and
UBSan).  Destruction releases once, a moved-from owner releases nothing, move-assignment releases the old handle first,
reset() on an empty owner does nothing, the growable buffer keeps its pointer up to its capacity and both growth policies ask
for the sizes the engine's and the channelizer's buffers always asked for."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_release_once_and_buffers_grow_as_before(tmp_path):
    exe = str(tmp_path / "hipres_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to load in front of it)
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "rtlsdrdiags_amd", "csrc"),
                    os.path.join(ROOT, "tests", "hipres", "hipres_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "hipres ok" in run.stdout, run.stdout
