"""The command-line tools (rtlsdrdiags_amd/bin/iqdemod_wide, _spectrum, _filter, _multi) as one table of named invocations
with their seeded inputs, and what each leaves behind: exit status, stderr, and the files under its output directory.

A case's arguments name its own directory as {d}: inputs are written to {d}/in, outputs are asked for under {d}/out (which
exists; {d}/out/none does not).  In the recorded stderr the directory reads <TMP> and the tool's own path (iqdemod_multi
prints argv[0]) reads <TOOL>.  Three tiers:
  cpu       refused before iqd_create: runs anywhere, the same with and without a GPU
  nodevice  reaches iqd_create: recorded where there is no GPU, and only compared there
  gpu       runs on the device: a few engine blocks each, every capture ending inside a call

tests/golden/tool_refusals.json holds the cpu and nodevice tiers ({status, stderr, files: {name: size}}), recorded on a machine
without a GPU; tests/golden/tool_transcripts.json the gpu tier ({status, stderr, files: {name: [size, sha256]}}), recorded on
an MI355X.  Both were recorded from the tools as they were before they were folded onto csrc/iqd_tool.h and
csrc/iqd_tool_chain.h:
  python -m tests.tool_cases refusals tests/golden/tool_refusals.json        (no GPU)
  python -m tests.tool_cases transcripts tests/golden/tool_transcripts.json  (on the GPU)"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rtlsdrdiags_amd", "bin")
RATE = 2048000
BLOCK = 32768                       # the engine's block, bytes per channel
TIMEOUT = 120                       # per process, as in the per-feature tool tests
STDOUT = "<stdout>"                 # iqdemod_filter's stream form writes there: recorded like a file


# ---- seeded inputs (bytes), each built once --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def band(n_samples, rate=RATE, seed=71):
    """tests/track_cases.chained_wide's two stations - FM at -700 kHz always on, AM at +250 kHz keyed on for the middle third"""
    from rtlsdrdiags_amd import synth
    from tests.detect_cases import STATIONS
    stations = [STATIONS[0], dict(STATIONS[1], on=[(n_samples / 3, 2 * n_samples / 3)])]
    return np.ascontiguousarray(synth.wideband(n_samples, float(rate), stations, seed=seed))


def wide_u8(blocks, m=8, tail=0, rate=RATE):
    """`blocks` engine blocks per channel of capture at decimation m (may be fractional: 2.5), then `tail` more bytes"""
    n = int(blocks * BLOCK * m) + tail
    return band((n + 1) // 2, rate)[:n].tobytes()


def wide_s8(blocks, tail=0):
    return (np.frombuffer(wide_u8(blocks, 8, tail), np.uint8) ^ 0x80).tobytes()


def wide_s16(blocks, tail=0):
    n = int(blocks * BLOCK * 16) + tail
    u = np.frombuffer(wide_u8(2 * blocks, 8, tail), np.uint8)[:(n + 1) // 2]
    return ((u.astype(np.int16) - 128) * 190).astype("<i2").tobytes()[:n]


def table_blocks(bins, frames, blocks, tail=0):
    n = 2 * bins * frames * blocks + tail
    return band((n + 1) // 2)[:n].tobytes()


def narrow(kind, n_bytes, seed):
    from rtlsdrdiags_amd import synth
    return getattr(synth, kind)((n_bytes + 1) // 2, seed=seed)[:n_bytes].tobytes()


def text(values, sep="\n"):
    return (sep.join("%.9g" % v if isinstance(v, float) else str(v) for v in values) + "\n").encode()


def window(n, top=12000):
    return [int(round(top * (0.5 - 0.5 * np.cos(2 * np.pi * (k + 0.5) / n)))) for k in range(n)]


def taps(n, seed):
    return [float(v) for v in np.random.default_rng(seed).uniform(-0.9, 0.9, n).astype(np.float32)]


def samples(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "i16":
        return np.where(rng.random(n) < 0.2, -32768, rng.integers(-32768, 32768, n)).astype("<i2").tobytes()
    return rng.normal(0, 3000, n).astype("<f4").tobytes()


# ---- the table ---------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, tool, args, tier, inputs, stdin):
        self.name, self.tool, self.args, self.tier, self.inputs, self.stdin = name, tool, args.split(), tier, inputs, stdin


CASES = []


def case(name, tool, args, tier="cpu", inputs=None, stdin=None):
    assert name not in {c.name for c in CASES}, name
    CASES.append(Case(name, "iqdemod_" + tool, args, tier, inputs or {}, stdin))


CAP = {"cap.iq": lambda: wide_u8(0.25)}                            # something to open, for the cases that get that far
W = "in={d}/in/cap.iq rate=2048000 "                               # iqdemod_wide: a capture and its rate
WC = W + "offsets=100000,-200000 modes=2,1 out={d}/out/p_%d.s16 "  # ... two fixed channels
WT = W + "tracks=2 bins=128 frames=64 modes=2 out={d}/out/p_%d.s16 "   # ... two track-following channels
SP = "in={d}/in/cap.iq rate=2048000 bins=64 frames=32 out={d}/out/pw.u32 "
CHAIN = "detect={d}/out/runs.txt track={d}/out/tracks.txt measure={d}/out/meas.txt events={d}/out/events.txt "

# iqdemod_wide: everything it can say before iqd_create, in the order main() gets there
case("wide.edges two numbers", "wide", WC + "edges=1,2")
case("wide.unknown first", "wide", "bogus=1 " + WC)
case("wide.unknown middle", "wide", W + "what offsets=100000 modes=2 out={d}/out/p_%d.s16")
case("wide.unknown last", "wide", WC + "offset=5")
case("wide.unknown before bad edges", "wide", WC + "nonsense edges=1")
case("wide.unknown after bad edges", "wide", WC + "edges=1 nonsense")
case("wide.modes= exact word only: modes=autox is a list", "wide", WC + "modes=autox")
case("wide.rate=2000000", "wide", "in={d}/in/cap.iq rate=2000000 offsets=0 modes=2 out={d}/out/p_%d.s16")
case("wide.rate=2000000 with decimation= passes the rate check", "wide", "rate=2000000 decimation=8")
case("wide.rate twice, the last wins", "wide", "rate=2048000 rate=2000000")
case("wide.rate below 2 x 256000", "wide", "rate=256000")
case("wide.format=u16", "wide", WC + "format=u16")
case("wide.format twice, the last wins", "wide", WC + "format=u16 format=s8 survey=0,1000,4")
case("wide.format=s8 survey=", "wide", WC + "format=s8 survey=0,1000,4 surveylog={d}/out/sv.txt")
case("wide.format=s16 scan=", "wide", WC + "format=s16 scan=1,2,3")
case("wide.format=s8 fractional", "wide", "in={d}/in/cap.iq rate=2400000 offsets=0 modes=2 out={d}/out/p_%d.s16 format=s8")
case("wide.format=s16 decimation=75/8", "wide", WC + "format=s16 decimation=75/8")
case("wide.agc=fast", "wide", WC + "agc=harris,fast")
case("wide.agc= empty", "wide", WC + "agc=")
case("wide.agc= trailing comma", "wide", WC + "agc=harris,")
case("wide.agc= scan=", "wide", WC + "agc=off,lowpass scan=1,2,3")
case("wide.agc= fractional", "wide", WC + "agc=harris decimation=75/8")
case("wide.rxgain= format=s16", "wide", WC + "rxgain=20 format=s16")
case("wide.agc=off alone follows nothing", "wide", WC + "agc=off,off scan=1,2")
case("wide.modes=auto without tracks=", "wide", W + "offsets=0 modes=auto out={d}/out/p_%d.s16")
case("wide.measlog= without tracks=", "wide", WC + "measlog={d}/out/m.txt")
case("wide.tracks=0x4 is base 10: no tracks", "wide", W + "tracks=0x4 modes=auto out={d}/out/p_%d.s16")
case("wide.tracks= scan=", "wide", WT + "scan=1,2,3")
case("wide.tracks= rxgain=", "wide", WT + "rxgain=10")
case("wide.tracks= fractional", "wide", WT + "decimation=75/8")
case("wide.tracks= format=s8", "wide", WT + "format=s8")
case("wide.tracks usage: offsets=", "wide", WT + "offsets=0")
case("wide.tracks usage: tracks=65", "wide", WT + "tracks=65")
case("wide.tracks usage: lag=2", "wide", WT + "lag=2")
case("wide.tracks usage: minstate=0", "wide", WT + "minstate=0")
case("wide.tracks usage: blocks=0x10 is atoi: 0", "wide", WT + "blocks=0x10")
case("wide.tracks geometry: no multiple of 64", "wide", WT + "bins=64 frames=1")
case("wide.tracks geometry: no multiple of 256", "wide", WT + "bins=64 frames=8 blocks=1")
case("wide.tracks cannot open", "wide", WT + "in={d}/in/none.iq")
case("wide.tracks cannot create pcm", "wide", WT + "out={d}/out/none/p_%d.s16", inputs=CAP)
case("wide.tracks cannot create tracklog", "wide", WT + "tracklog={d}/out/none/t.txt", inputs=CAP)
case("wide.survey= scan=", "wide", W + "survey=0,1000,4 surveylog={d}/out/sv.txt scan=1,2,3")
case("wide.usage: nothing", "wide", "")
case("wide.usage: offsets= empty", "wide", W + "offsets= modes=2 out={d}/out/p_%d.s16")
case("wide.usage: gains= empty", "wide", WC + "gains=")
case("wide.usage: no out=", "wide", W + "offsets=0 modes=2")
case("wide.usage: survey count 4097", "wide", W + "survey=0,1000,4097 surveylog={d}/out/sv.txt")
case("wide.usage: survey without surveylog=", "wide", W + "survey=0,1000,4")
case("wide.usage: surveyshift=9", "wide", W + "survey=0,1000,4 surveyshift=9 surveylog={d}/out/sv.txt")
case("wide.usage: scan= two numbers", "wide", WC + "scan=1,2")
case("wide.usage: decimation=8/0", "wide", WC + "decimation=8/0")
case("wide.usage: decimation=1", "wide", WC + "decimation=1")
case("wide.usage: blocks=abc", "wide", WC + "blocks=abc")
case("wide.survey offset outside", "wide", W + "survey=1000000,8000,4 surveylog={d}/out/sv.txt")
case("wide.offset outside", "wide", W + "offsets=0,-1024000 modes=2 out={d}/out/p_%d.s16")
case("wide.cannot open", "wide", WC + "in={d}/in/none.iq")
case("wide.cannot create pcm", "wide", W + "offsets=0,1000 modes=2 out={d}/out/none/p_%d.s16", inputs=CAP)
case("wide.cannot create surveylog", "wide", WC + "survey=0,1000,4 surveylog={d}/out/none/sv.txt", inputs=CAP)
case("wide.cannot create freqlog", "wide", WC + "freqlog={d}/out/none/f.txt", inputs=CAP)
case("wide.cannot create gainlog", "wide", WC + "gainlog={d}/out/none/g.txt freqlog={d}/out/f.txt", inputs=CAP)
# ... and which message wins where two apply
case("wide.both: format=s8 scan= tracks= -> format", "wide", WT + "format=s8 scan=1,2,3")
case("wide.both: format=u16 agc=fast -> format", "wide", WC + "format=u16 agc=fast")
case("wide.both: rate=2000000 format=u16 -> rate", "wide", "rate=2000000 format=u16")
case("wide.both: agc=harris scan= tracks= -> agc", "wide", WT + "agc=harris scan=1,2,3")
case("wide.both: format=s16 rxgain= -> agc", "wide", WC + "format=s16 rxgain=3")
case("wide.both: modes=auto survey= scan= -> needs tracks", "wide", W + "modes=auto survey=0,1000,4 scan=1,2,3")
case("wide.both: tracks= offsets= scan= -> tracks with scan", "wide", WT + "offsets=0 scan=1,2,3")
case("wide.both: tracks usage before geometry", "wide", WT + "bins=64 frames=1 lag=2")
case("wide.both: survey= scan= without in= -> survey with scan", "wide", "rate=2048000 survey=0,1000,4 scan=1,2,3")
case("wide.both: survey offset before offset", "wide", W + "offsets=2000000 modes=2 out={d}/out/p_%d.s16 survey=1000000,8000,4 surveylog={d}/out/s.txt")
case("wide.both: offset outside before cannot open", "wide", WC + "in={d}/in/none.iq offsets=1024000")
case("wide.both: cannot open before cannot create", "wide", WC + "in={d}/in/none.iq out={d}/out/none/p_%d.s16")
case("wide.no device", "wide", WC + "freqlog={d}/out/f.txt gainlog={d}/out/g.txt survey=0,1000,4 surveylog={d}/out/sv.txt", "nodevice", CAP)
case("wide.tracks no device", "wide", WT + "tracklog={d}/out/t.txt measlog={d}/out/m.txt", "nodevice", CAP)

# iqdemod_spectrum
case("spectrum.edges empty", "spectrum", SP + "edges=")
case("spectrum.unknown first", "spectrum", "rates=1 " + SP)
case("spectrum.unknown after bad edges", "spectrum", SP + "edges=1,2 what")
case("spectrum.unknown last", "spectrum", SP + "slot=3")
case("spectrum.usage: nothing", "spectrum", "")
case("spectrum.usage: format=s16", "spectrum", SP + "format=s16")
case("spectrum.usage: frames=2^24+1", "spectrum", SP + "frames=16777217")
case("spectrum.usage: bins=0x40 is base 10: 0", "spectrum", SP + "bins=0x40")
case("spectrum.usage: rate=0", "spectrum", SP + "rate=0")
case("spectrum.bins twice, the last wins", "spectrum", SP + "bins=0 bins=64 window={d}/in/none.txt")
case("spectrum.events= without measure=", "spectrum", SP + "detect={d}/out/r.txt track={d}/out/t.txt events={d}/out/e.txt")
case("spectrum.measure= without track=", "spectrum", SP + "detect={d}/out/r.txt measure={d}/out/m.txt")
case("spectrum.track= without detect=", "spectrum", SP + "track={d}/out/t.txt")
case("spectrum.detect= rate=2048000.5", "spectrum", SP + "detect={d}/out/r.txt rate=2048000.5")
case("spectrum.detect= rate=2^32", "spectrum", SP + "detect={d}/out/r.txt rate=4294967296")
case("spectrum.window of 63", "spectrum", SP + "window={d}/in/w.txt", inputs={"w.txt": lambda: text(window(63))})
case("spectrum.window holds 40000", "spectrum", SP + "window={d}/in/w.txt", inputs={"w.txt": lambda: text(window(63) + [40000], ", ")})
case("spectrum.window holds 12x", "spectrum", SP + "window={d}/in/w.txt", inputs={"w.txt": lambda: text(window(63) + ["12x"], ",")})
case("spectrum.window missing", "spectrum", SP + "window={d}/in/none.txt")
case("spectrum.cannot open in", "spectrum", SP + "in={d}/in/none.iq log={d}/out/log.txt")
case("spectrum.cannot create out", "spectrum", SP + "out={d}/out/none/pw.u32 log={d}/out/log.txt", inputs=CAP)
case("spectrum.cannot create events", "spectrum", SP + CHAIN + "events={d}/out/none/e.txt", inputs=CAP)
case("spectrum.both: usage before events= needs", "spectrum", "events={d}/out/e.txt")
case("spectrum.both: events= and measure= without track= -> events", "spectrum", SP + "detect={d}/out/r.txt measure={d}/out/m.txt events={d}/out/e.txt")
case("spectrum.both: measure= without track= or detect= -> measure", "spectrum", SP + "measure={d}/out/m.txt")
case("spectrum.both: rate before window", "spectrum", SP + "detect={d}/out/r.txt rate=0.5 window={d}/in/none.txt")
case("spectrum.both: window before files", "spectrum", SP + "in={d}/in/none.iq window={d}/in/none.txt")
case("spectrum.no device", "spectrum", SP + CHAIN + "log={d}/out/log.txt", "nodevice", CAP)

# iqdemod_filter
FI = "kind=fir_i16 taps={d}/in/h.txt "
H = {"h.txt": lambda: text(taps(8, 5))}
case("filter.unknown first", "filter", "tap=1 " + FI)
case("filter.unknown last", "filter", FI + "chunks=4")
case("filter.usage: nothing", "filter", "")
case("filter.usage: kind=fir", "filter", "kind=fir taps={d}/in/h.txt")
case("filter.usage: chunk=0", "filter", FI + "chunk=0")
case("filter.usage: chunk=2^31", "filter", FI + "chunk=2147483648")
case("filter.usage: channels= without out=", "filter", FI + "channels=2 in={d}/in/x_%d.raw")
case("filter.usage: in= without channels=", "filter", FI + "in={d}/in/x_%d.raw")
case("filter.kind twice, the last wins", "filter", "kind=fir_i16 kind=fir taps={d}/in/h.txt")
case("filter.taps empty", "filter", FI, inputs={"h.txt": lambda: b""})
case("filter.taps only separators", "filter", FI, inputs={"h.txt": lambda: b" ,\n, \n"})
case("filter.taps missing", "filter", FI)
case("filter.den empty", "filter", "kind=iir_f32 taps={d}/in/h.txt den={d}/in/a.txt", inputs=dict(H, **{"a.txt": lambda: b"\n"}))
case("filter.cannot open channel 1", "filter", FI + "channels=2 in={d}/in/x_%d.raw out={d}/out/y_%d.raw",
     inputs=dict(H, **{"x_0.raw": lambda: samples("i16", 100, 1)}))
case("filter.cannot create channel 0", "filter", FI + "channels=1 in={d}/in/x_%d.raw out={d}/out/none/y_%d.raw",
     inputs=dict(H, **{"x_0.raw": lambda: samples("i16", 100, 1)}))
case("filter.both: usage before taps", "filter", "kind=fir taps={d}/in/none.txt")
case("filter.both: taps before den", "filter", FI + "den={d}/in/none.txt", inputs={"h.txt": lambda: b""})
case("filter.both: taps before the files", "filter", FI + "channels=1 in={d}/in/none_%d.raw out={d}/out/y_%d.raw")
case("filter.no device", "filter", FI, "nodevice", H, stdin=lambda: samples("i16", 100, 1))
case("filter.no device, files", "filter", FI + "channels=1 in={d}/in/x_%d.raw out={d}/out/y_%d.raw", "nodevice",
     dict(H, **{"x_0.raw": lambda: samples("i16", 100, 1)}))

# iqdemod_multi: it makes its engine before it opens a file
MU = "channels=2 in={d}/in/cap_%d.iq out={d}/out/pcm_%d.s16 "
case("multi.usage: nothing", "multi", "")
case("multi.usage: unknown", "multi", MU + "nonsense")
case("multi.usage: layout=file", "multi", MU + "layout=file")
case("multi.usage: channels=0x2 is atoi: 0", "multi", "channels=0x2 in={d}/in/cap_%d.iq out={d}/out/pcm_%d.s16")
case("multi.usage: modes= empty", "multi", MU + "modes=")
case("multi.usage: blocks=0", "multi", MU + "blocks=0")
case("multi.no device", "multi", MU, "nodevice", {"cap_0.iq": lambda: narrow("fm_tone", BLOCK, 3), "cap_1.iq": lambda: narrow("am_tone", BLOCK, 4)})

# ---- on the device -------------------------------------------------------------------------------------------------------------
# iqdemod_wide: calls of 4 engine blocks; 6 blocks and 37 units of 512 bytes and 100 bytes more end as 2 whole blocks, one short
# block, and a rest below one unit that is cut off
U8 = {"cap.iq": lambda: wide_u8(6, 8, 512 * 37 + 100)}
case("wide.integer rate", "wide", "in={d}/in/cap.iq decimation=8 rate=2048000 offsets=-636000,250000 modes=2,1 out={d}/out/p_%d.s16 "
     "freqlog={d}/out/f.txt squelch=-45,-60 rotation=1", "gpu", U8)
case("wide.rotation=0 gains=", "wide", W + "offsets=-700000,250000,10000 modes=2,1,5 gains=1,0 rotation=0 blocks=3 out={d}/out/p_%d.s16", "gpu", U8)
case("wide.fractional rate", "wide", "in={d}/in/cap.iq rate=2400000 offsets=-636000,250000 modes=2,1 out={d}/out/p_%d.s16 blocks=2 freqlog={d}/out/f.txt",
     "gpu", {"cap.iq": lambda: wide_u8(3, 75 / 8, 4800 * 5 + 77, rate=2400000)})
case("wide.format=s8", "wide", WC + "format=s8 blocks=2", "gpu", {"cap.iq": lambda: wide_s8(3, 512 * 9 + 5)})
case("wide.format=s16", "wide", WC + "format=s16 blocks=2 gains=0,2", "gpu", {"cap.iq": lambda: wide_s16(3, 1024 * 9 + 6)})
case("wide.scan", "wide", W + "offsets=100000,-200000,364000 modes=2,1 centre=100000000 scan=99336000,100336000,100000,0,0,0 squelch=-50,-40 "
     "freqlog={d}/out/f.txt out={d}/out/p_%d.s16", "gpu", U8)
case("wide.survey alone", "wide", W + "survey=-800000,50000,33 surveyshift=2 surveylog={d}/out/sv.txt", "gpu", U8)
case("wide.survey with offsets", "wide", WC + "survey=-800000,100000,17 surveylog={d}/out/sv.txt blocks=2", "gpu", U8)
# (rate 9/2 x 256 kS/s: a short block of 5 units of 64 x 9 bytes has 640 row bytes, no multiple of 256)
case("wide.survey, short block not surveyed", "wide", "in={d}/in/cap.iq rate=1152000 survey=-400000,50000,17 surveylog={d}/out/sv.txt blocks=2",
     "gpu", {"cap.iq": lambda: wide_u8(3, 9 / 2, 576 * 5 + 77, rate=1152000)})
case("wide.agc with gainlog", "wide", WC + "agc=harris,off gainlog={d}/out/g.txt blocks=2", "gpu", U8)
case("wide.rxgain", "wide", WC + "rxgain=20 gainlog={d}/out/g.txt freqlog={d}/out/f.txt", "gpu", U8)
# tracks=: table blocks of 128 x 64 samples, row 2048 bytes; calls of 8; 19 whole blocks and 300 bytes end as a call of 3
TB = {"cap.iq": lambda: table_blocks(128, 64, 19, 300)}
TR = W + "tracks=3 bins=128 frames=64 blocks=8 lag=1 minwidth=1 open=1 out={d}/out/p_%d.s16 "
case("wide.tracks", "wide", TR + "modes=2,1 gains=2,3 tracklog={d}/out/t.txt squelch=-60", "gpu", TB)
case("wide.tracks modes=auto", "wide", TR + "modes=auto tracklog={d}/out/t.txt measlog={d}/out/m.txt minsum=1", "gpu", TB)
case("wide.tracks measlog alone, lag=0 minstate=1", "wide", TR + "modes=2 lag=0 minstate=1 measlog={d}/out/m.txt tracklog={d}/out/t.txt bias=0x10 edges=2,4,8", "gpu", TB)
case("wide.tracks cannot create measlog", "wide", TR + "modes=2 measlog={d}/out/none/m.txt", "gpu", TB)
case("wide.library refuses gains=9", "wide", WC + "gains=9", "gpu", U8)
case("wide.tracks library refuses bins=100", "wide", TR.replace("bins=128", "bins=100") + "modes=2", "gpu", TB)

# iqdemod_spectrum: 11 blocks and a part of one
SB = {"cap.iq": lambda: table_blocks(64, 32, 11, 1234), "w.txt": lambda: text(window(64), ", ")}
SB128 = {"cap.iq": lambda: table_blocks(128, 64, 19, 300)}
case("spectrum.plain", "spectrum", SP + "log={d}/out/log.txt window={d}/in/w.txt", "gpu", SB)
case("spectrum.format=s8", "spectrum", SP + "format=s8", "gpu", {"cap.iq": lambda: (np.frombuffer(table_blocks(64, 32, 11, 1234), np.uint8) ^ 0x80).tobytes()})
case("spectrum.band chain", "spectrum", "in={d}/in/cap.iq rate=2048000 bins=128 frames=64 out={d}/out/pw.u32 log={d}/out/log.txt " + CHAIN +
     "maxdet=1 minwidth=1 open=1 slots=3 minsum=1 minactive=1 votemin=1", "gpu", SB128)
case("spectrum.band chain, defaults", "spectrum", "in={d}/in/cap.iq rate=2048000 bins=128 frames=64 out={d}/out/pw.u32 " + CHAIN, "gpu", SB128)
case("spectrum.band chain, every key", "spectrum", "in={d}/in/cap.iq rate=2048000 bins=128 frames=64 out={d}/out/pw.u32 " + CHAIN +
     "rank=70 ratio_q8=1024 guard=2 bridge=4 minwidth=2 maxdet=4 slots=2 gate_q8=400 open=2 hold=1 alpha_q8=128 bias=0x20 edges=2,5,9 "
     "margin=2 beta_q16=600 carrier=2 minsum=16 carrier_q8=100 wide=6 minactive=1 votemin=2 maxevents=1", "gpu", SB128)
case("spectrum.detect only", "spectrum", SP + "detect={d}/out/runs.txt minwidth=1", "gpu", SB)
case("spectrum.library refuses bins=100", "spectrum", SP + "bins=100", "gpu", SB)
case("spectrum.library refuses votemin=0", "spectrum", "in={d}/in/cap.iq rate=2048000 bins=128 frames=64 out={d}/out/pw.u32 " + CHAIN + "votemin=0", "gpu", SB128)

# iqdemod_filter: each kind from stdin to stdout, and two channels of unequal length over files
IIR = {"b.txt": lambda: text([0.2, 0.3, 0.1], ", "), "a.txt": lambda: text([-0.5, 0.25], " ")}
H24 = {"h.txt": lambda: text(taps(24, 8), ",\n")}
case("filter.decimate_i16", "filter", "kind=decimate_i16 taps={d}/in/h.txt factor=4 chunk=777", "gpu", H24, lambda: samples("i16", 5001, 2))
case("filter.fir_i16", "filter", "kind=fir_i16 taps={d}/in/h.txt chunk=1000", "gpu", H24, lambda: samples("i16", 3000, 3))
case("filter.fir_f32", "filter", "kind=fir_f32 taps={d}/in/h.txt", "gpu", H24, lambda: samples("f32", 3000, 4))
case("filter.iir_f32", "filter", "kind=iir_f32 taps={d}/in/b.txt den={d}/in/a.txt chunk=64", "gpu", IIR, lambda: samples("f32", 1000, 5))
case("filter.two channels of unequal length", "filter", "kind=decimate_i16 taps={d}/in/h.txt factor=3 channels=2 in={d}/in/x_%d.raw out={d}/out/y_%d.raw chunk=1001",
     "gpu", dict(H24, **{"x_0.raw": lambda: samples("i16", 4000, 6), "x_1.raw": lambda: samples("i16", 2500, 7)}))
case("filter.library refuses factor=0", "filter", "kind=decimate_i16 taps={d}/in/h.txt factor=0", "gpu", H24, lambda: samples("i16", 100, 2))

# iqdemod_multi: calls of 2 blocks
M2 = {"cap_0.iq": lambda: narrow("fm_tone", 5 * BLOCK + 640 + 13, 3), "cap_1.iq": lambda: narrow("am_tone", BLOCK + 320, 4)}
case("multi.files of unequal length", "multi", MU + "modes=2,1 blocks=2 rotation=1,0 threshold=-60", "gpu", M2)
case("multi.interleaved", "multi", "channels=2 in={d}/in/cap.iq out={d}/out/pcm_%d.s16 layout=files layout=interleaved modes=3,2 blocks=2",
     "gpu", {"cap.iq": lambda: narrow("fm_tone", 7 * BLOCK + 1000, 5)})
case("multi.agc=1", "multi", MU + "agc=1 blocks=2", "gpu", M2)
case("multi.cannot open capture 1", "multi", MU, "gpu", {"cap_0.iq": lambda: narrow("fm_tone", BLOCK, 3)})
case("multi.cannot create", "multi", "channels=2 in={d}/in/cap_%d.iq out={d}/out/none/pcm_%d.s16", "gpu", M2)


# ---- running -----------------------------------------------------------------------------------------------------------------
def run_case(c, tmp_root, hashes):
    d = os.path.join(str(tmp_root), "c%03d" % CASES.index(c))
    os.makedirs(os.path.join(d, "in"))
    os.makedirs(os.path.join(d, "out"))
    for name, make in c.inputs.items():
        with open(os.path.join(d, "in", name), "wb") as f:
            f.write(make())
    tool = os.path.join(BIN, c.tool)
    r = subprocess.run([tool] + [a.replace("{d}", d) for a in c.args], input=c.stdin() if c.stdin else b"", capture_output=True, timeout=TIMEOUT)
    files = {}
    for dirpath, _, names in os.walk(os.path.join(d, "out")):
        for n in names:
            with open(os.path.join(dirpath, n), "rb") as f:
                files[os.path.relpath(os.path.join(dirpath, n), os.path.join(d, "out"))] = f.read()
    if c.stdin:
        files[STDOUT] = r.stdout
    else:
        assert r.stdout == b"", (c.name, r.stdout[:200])
    return dict(status=r.returncode, stderr=r.stderr.decode().replace(d, "<TMP>").replace(tool, "<TOOL>"),
                files={k: [len(v), hashlib.sha256(v).hexdigest()] if hashes else len(v) for k, v in files.items()})


def collect(tmp_root, tiers, hashes):
    """{case name: {status, stderr, files}} of every case of `tiers`, one process at a time"""
    return {c.name: run_case(c, tmp_root, hashes) for c in CASES if c.tier in tiers}


def dump(table):
    return json.dumps(table, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    import tempfile
    tiers, hashes = {"refusals": (("cpu", "nodevice"), False), "transcripts": (("gpu",), True)}[sys.argv[1]]
    with tempfile.TemporaryDirectory() as tmp:
        got = collect(tmp, tiers, hashes)
    with open(sys.argv[2], "w") as f:
        f.write(dump(got))
    print("%d cases -> %s" % (len(got), sys.argv[2]))
