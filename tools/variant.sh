#!/bin/bash
# Builds a diagnostic or A/B variant of libiqdemod.so into tmp_variants/lib_<name>.so:
#   tools/variant.sh <name> [-DFLAG=1 ...]
# The flags go to every translation unit, through the library's own Makefile (rtlsdrdiags_amd/csrc/Makefile, EXTRA=...):
# the switch names are per kernel, and iqd_stream_mixed.hip compiles the WBFM stream bodies a second time.  Only the library
# is built, the shipped one is left alone.  Every variant is a full build (one hipcc run over all translation units): 2 min 14 s
# on the 8-core machine it was last timed on.
# Load it with IQD_LIB=tmp_variants/lib_<name>.so (tools/ab.sh, tools/abn.sh, the *_probe.py scripts).
# The build switches that remain and the tool that reads each: DESIGN.md, 4.9.
set -e
[ $# -ge 1 ] || { echo "usage: tools/variant.sh <name> [-DFLAG=1 ...]" >&2; exit 2; }
NAME=$1; shift
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "$ROOT/tmp_variants"
make -C "$ROOT/rtlsdrdiags_amd/csrc" OUT="../../tmp_variants/lib_$NAME.so" EXTRA="$*" "../../tmp_variants/lib_$NAME.so"
echo built tmp_variants/lib_$NAME.so
