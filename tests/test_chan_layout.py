"""CPU tier: the channelizer's layout code (rtlsdrdiags_amd/csrc/iqd_chan_layout.cpp with iqd_chan_design.cpp, no HIP call in
either) in a stand-alone program (tests/chan_layout/chan_layout_check.cpp, built here with AddressSanitizer and UBSan).  Every
A-operand byte unpacks to the tap it came from at K = 1, 31, 32, 33, 257 and 1024 Q for Q = 1, 2, 4, 8, padding is zero and the
S16 row sums are the rows' sums; mixed kinds over 1, 2 and 5 sources with 1, 8, 9 and 65 channels of a kind on a source put
every channel in exactly one slot, one source and one kind in a tile, the kinds in order, and every tile in exactly one
workgroup row of its kind; the upload pieces after a retune name exactly the dirty tiles, after a source change everything."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")


def test_packing_grouping_and_upload_pieces(tmp_path):
    exe = str(tmp_path / "chan_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to load in front of it)
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "chan_layout", "chan_layout_check.cpp"), os.path.join(CSRC, "iqd_chan_layout.cpp"),
                    os.path.join(CSRC, "iqd_chan_design.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "chan layout ok" in run.stdout, run.stdout
