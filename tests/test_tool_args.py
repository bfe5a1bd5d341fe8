"""CPU tier: the part of the command-line tools that needs no library (rtlsdrdiags_amd/csrc/iqd_tool.h: the key= table, the list
splitter, the number-file reader, channelName, the file owner and the band chain's arguments with derive()) in a stand-alone
program (tests/tool_args/tool_args_check.cpp, built here with AddressSanitizer and UBSan).  The table against hand-written
expectations for each tool's kinds of rows - a repeated key, the whole words, an unknown key first, in the middle and last,
each conversion on odd input; the splitter on "", "1", "1,", ",1" and "a,2"; the reader on comma and white-space mixes, tokens
out of range and empty files; a 4000-character pattern; derive() at every N with and without each key that overrides it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")


def test_table_lists_numbers_names_and_derive(tmp_path):
    exe = str(tmp_path / "tool_args_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to load in front of it)
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tool_args", "tool_args_check.cpp"), "-o", exe], check=True)
    work = tmp_path / "files"
    work.mkdir()
    run = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "tool args ok" in run.stdout, run.stdout
