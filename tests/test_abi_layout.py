"""CPU tier: the layout of every public struct of include/iqdemod.h, as the C compiler sees it, against the Python binding's
mirror of it (rtlsdrdiags_amd/capi.py: a ctypes.Structure or a numpy dtype).  A stand-alone C99 program
(tests/abi_layout/abi_layout_check.c, built here) prints sizeof and every field's offsetof and size; its field lists are held
against the header's own, so that neither a struct nor a field of the header can go unchecked, and every line against the
mirror - size, field names and order, offsets, field sizes.  No library call, no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from rtlsdrdiags_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIRROR = {
    "iqd_config": capi.Config, "iqd_agc_state": capi.AgcState, "iqd_stats": capi.Stats,
    "iqd_channelizer_config": capi.ChannelizerConfig, "iqd_spectrum_config": capi.SpectrumConfig,
    "iqd_detect_config": capi.DetectConfig, "iqd_detect_row": capi.DETECT_ROW, "iqd_detection": capi.DETECTION,
    "iqd_track_config": capi.TrackConfig, "iqd_track_slot": capi.TRACK_SLOT, "iqd_track_block": capi.TRACK_BLOCK,
    "iqd_track_follow": capi.TrackFollow, "iqd_measure_config": capi.MeasureConfig, "iqd_track_measure": capi.TRACK_MEASURE,
    "iqd_tracklog_config": capi.TrackLogConfig, "iqd_track_summary": capi.TRACK_SUMMARY,
    "iqd_tracklog_counts": capi.TRACKLOG_COUNTS,
}


def header_structs():
    """{struct name: [field names in order]} of every `typedef struct iqd_* { ... }` of the header"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "iqdemod.h")).read(), flags=re.S)
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(iqd_\w+)\s*\{(.*?)\}", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")                       # "uint32_t n_measured, votes[3]": the type stands once
            fields += [re.search(r"(\w+)\s*(\[\d+\])?\s*$", d).group(1) for d in [first] + more]
        out[name] = fields
    return out


def compiled_layout(tmp_path):
    """{struct name: (sizeof, [(field, offset, size), ...])} as abi_layout_check prints it"""
    exe = str(tmp_path / "abi_layout_check")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi_layout", "abi_layout_check.c"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, check=True, text=True)
    out = {}
    for line in run.stdout.splitlines():
        what, a, *b = line.split()
        if what == "struct":
            out[a] = (int(b[0]), [])
        else:
            name, field = what.split(".")
            out[name][1].append((field, int(a), int(b[0])))
    return out


def mirror_layout(m):
    """(size, [(field, offset, size), ...]) of a ctypes.Structure or a numpy structured dtype"""
    if isinstance(m, np.dtype):
        return m.itemsize, [(k, m.fields[k][1], m.fields[k][0].itemsize) for k in m.names]
    return C.sizeof(m), [(k, getattr(m, k).offset, getattr(m, k).size) for k, _ in m._fields_]


def test_every_public_struct_matches_its_mirror(tmp_path):
    header, compiled = header_structs(), compiled_layout(tmp_path)
    assert len(header) == 17 and set(header) == set(MIRROR), sorted(set(header) ^ set(MIRROR))   # a struct without a mirror fails
    assert sum(isinstance(m, np.dtype) for m in MIRROR.values()) == 7
    assert list(compiled) == list(header)                                                      # ... or without its lines
    for name, fields in header.items():
        size, lines = compiled[name]
        assert [f for f, _, _ in lines] == fields, name                  # the program leaves no field of the header out
        assert lines[-1][1] + lines[-1][2] <= size
        assert mirror_layout(MIRROR[name]) == (size, lines), name
