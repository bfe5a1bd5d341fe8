"""The small calls that the planner (iqd_plan.cpp: plan_call) runs as ONE launch, and their neighbours that it does not: the
shapes tests/test_gpu_one_launch.py runs on the device, pinned on the CPU tier by tests/test_host_planning.py through the
host planning binding (256 CUs) - so a planner change that would make the GPU cases vacuous fails without a GPU first.

A shape is the row length and the channels per family; the AM / FM / SSB channels' rotation selectors cycle +1 / 0 / -1
inside each family, the WBFM family has one selector (chosen per case: the plan does not depend on which) unless the shape
gives its channels per selector.  Every fused shape here has 768-sample segments, workgroups of three rings and one round."""
import collections

FAMS = ("am", "fm", "wbfm", "ssb")
SELECTORS = (1, 0, -1)                 # the order of FamilyShape::rot_count: +Fs/4, none, -Fs/4
PLAN_STREAM = 1
MIX = {"am": 20, "fm": 20, "wbfm": 20, "ssb": 40}

Shape = collections.namedtuple("Shape", "name n counts fused mix_wgs grid segs wbfm_rots bounded epochs")
SHAPES = collections.OrderedDict()


def _add(name, n, counts, fused, mix_wgs=0, grid=None, segs=0, wbfm_rots=None, bounded=True, epochs=False):
    counts = {f: int(counts.get(f, 0)) for f in FAMS}
    SHAPES[name] = Shape(name, n, counts, fused, mix_wgs, grid or {}, segs, wbfm_rots, bounded, epochs)


def cycle_counts(n):
    """channels per selector of a family whose k-th channel has selector SELECTORS[k % 3]"""
    return ((n + 2) // 3, (n + 1) // 3, n // 3)


def plan_fams(s, wbfm_rot=1):
    """plan_call's description of the shape's families"""
    fams = {}
    for f in FAMS:
        n = s.counts[f]
        if not n:
            continue
        if f == "wbfm":
            rc = s.wbfm_rots or tuple(n if r == wbfm_rot else 0 for r in SELECTORS)
            fams[f] = (tuple(rc), s.bounded, s.epochs)
        else:
            fams[f] = (cycle_counts(n), True, False)
    return fams


def hold(plan_call, s, wbfm_rot=1, gated=False, flags=0):
    """Holds the shape to the planner; returns (the plan, the families on a streaming pipeline)."""
    p = plan_call(s.n, plan_fams(s, wbfm_rot), flags=flags, gated=gated)
    tag = (s.name, wbfm_rot, gated, flags)
    present = [f for f in FAMS if s.counts[f]]
    assert p["fused"] == s.fused, (tag, p)
    streams = sum(p["fam"][f]["path"] == PLAN_STREAM for f in present)
    if not s.fused:
        assert streams == 0, (tag, p)            # (calls this small take their tile kernels when they are not one launch)
        return p, streams
    assert p["mix_wgs"] == s.mix_wgs, (tag, p["mix_wgs"])
    for f in present:
        q = p["fam"][f]
        assert (q["path"], q["rings"], q["rounds"]) == (PLAN_STREAM, 3, 1), (tag, f, q)
        assert (q["grid"], q["tiles_per_ch"], q["tile_len"]) == (s.grid[f], s.segs, 768), (tag, f, q)
        assert q["lead_shift"] == 0, (tag, f, q)
    if s.counts["wbfm"]:
        assert not p["fam"]["wbfm"]["grouped"] and not p["fam"]["wbfm"]["epochs"], (tag, p["fam"]["wbfm"])
    assert sum(s.grid[f] for f in present) == s.mix_wgs
    return p, streams


# ---- the 100-channel mix (20 AM + 20 FM + 20 WBFM + 40 SSB) by row length ---------------------------------------------
_G14 = {"wbfm": 3, "fm": 3, "ssb": 5, "am": 3}
_add("mix", 1 << 14, MIX, True, 14, _G14, 22)
_add("mix_16512", 16512, MIX, True, 14, _G14, 22)             # last segment 384 samples
_add("mix_17024", 17024, MIX, True, 14, _G14, 23)             # last segment 128 samples: shorter than the lead-in
_add("mix_32768", 1 << 15, MIX, True, 24, {"wbfm": 5, "fm": 5, "ssb": 9, "am": 5}, 43)
_add("mix_49152", 49152, MIX, True, 35, {"wbfm": 7, "fm": 7, "ssb": 14, "am": 7}, 64)      # a channel fills a ring exactly
_add("mix_82176", 82176, MIX, True, 59, {"wbfm": 12, "fm": 12, "ssb": 23, "am": 12}, 107)
ROW_LENGTHS = ("mix", "mix_16512", "mix_17024", "mix_32768", "mix_49152", "mix_82176")

# ---- family subsets, 40 channels per family present (every one of the eleven is one launch at 40) ---------------------
SUBSET_CHANNELS = 40
SUBSETS = []
for _bits in range(1, 16):
    _names = [f for k, f in enumerate(FAMS) if _bits >> k & 1]
    if len(_names) < 2:
        continue
    _name = "subset_" + "_".join(_names)
    _add(_name, 1 << 14, {f: SUBSET_CHANNELS for f in _names}, True, 5 * len(_names), {f: 5 for f in _names}, 22)
    SUBSETS.append(_name)

# ---- no smallest WBFM family exists: plan_call's size rule weighs the CALL (vlen x cost against the CUs), not a family, so beside
# 60 + 60 + 120 channels ONE WBFM channel is still a range of the one launch - the launch's last workgroup, 22 segments in one
# ring and two rings with none - and there is no w below which the call leaves it.  Without the channel: three families.
_G3 = {"ssb": 14, "fm": 7, "am": 7}
SMALLEST_WBFM = 1
_add("wbfm_1", 1 << 14, {"am": 60, "fm": 60, "wbfm": SMALLEST_WBFM, "ssb": 120}, True, 29, dict(_G3, wbfm=1), 22)
_add("wbfm_0", 1 << 14, {"am": 60, "fm": 60, "wbfm": 0, "ssb": 120}, True, 28, _G3, 22)
# ... the boundary that does exist: the smallest mix m + m + m + 2 m that is one launch, and the one below it
SMALLEST_MIX = 18
_add("mix_x18", 1 << 14, {"am": 18, "fm": 18, "wbfm": 18, "ssb": 36}, True, 14, _G14, 22)
_add("mix_x17", 1 << 14, {"am": 17, "fm": 17, "wbfm": 17, "ssb": 34}, False)

# ---- what takes the 100-channel mix off the one launch (calls this small then run their tile kernels) -----------------
_add("mix_two_selectors", 1 << 14, MIX, False, wbfm_rots=(10, 10, 0))
_add("mix_short_block", (1 << 14) - 64, MIX, False)           # not whole 128-sample units
_add("mix_unbounded_gain", 1 << 14, MIX, False, bounded=False, epochs=True)
_add("mix_gain_change_in_reach", 1 << 14, MIX, False, epochs=True)
