"""Which SIMD each wave of a WBFM streaming workgroup sits on (a build with -DIQD_ST_TIMING=1, see iqd_stream.hip):
    tools/variant.sh timing -DIQD_ST_TIMING=1
    IQD_LIB=tmp_variants/lib_timing.so python3 tools/simd_of_waves.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtlsdrdiags_amd import capi, synth

eng = capi.Engine(1, flags=0x4)
eng.set_mode("wbfm")
eng.accept(synth.fm_tone(1 << 20, seed=1))
st = eng.debug_stamps_ext(20016)[20000:]
print("wave: SIMD  " + "  ".join("%d:%d" % (w, int(v) - 1) for w, v in enumerate(st)))
by_simd = {}
for w, v in enumerate(st):
    by_simd.setdefault(int(v) - 1, []).append(w)
print("waves 0-2 are the IIR waves, 3-14 the P waves, 15 the audio wave;  by SIMD:", by_simd)
