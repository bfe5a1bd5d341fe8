"""CPU tier: the order in which the binding destroys what hangs off an engine, with a recording stand-in for the library (no
library is loaded, nothing runs on a GPU).  Every iqd_<kind>_destroy works on its engine's device and stream, so for each
of the nine kinds: Engine.close() destroys the child before the engine, and neither a later close() nor the child's end makes
another call; a child closed or dropped first is destroyed once, by itself."""
import gc

import numpy as np
import pytest

from rtlsdrdiags_amd import capi

MAKE = {
    "resampler": lambda e: capi.Resampler(e, "decimate_f32", np.ones(8), 2),
    "filter": lambda e: capi.Filter(e, "fir_f32", np.ones(8)),
    "gather": lambda e: capi.Gatherer(e, bytes(128), 0, 1),
    "channelizer": lambda e: capi.Channelizer(e, 4, 1),
    "spectrum": lambda e: capi.Spectrum(e, 64),
    "detect": lambda e: capi.Detector(e, 64),
    "track": lambda e: capi.Tracker(e, 64),
    "measure": lambda e: capi.Measure(e, 64),
    "tracklog": lambda e: capi.TrackLog(e),
}


class Recorder:
    """In place of the loaded library: every function exists, notes its name and reports success; a create hands out a handle."""

    def __init__(self):
        self.calls, self.handles = [], 0

    def __getattr__(self, name):
        if name not in capi.PROTOTYPES:
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(name)
            if name.endswith("create"):
                self.handles += 1
                args[-1]._obj.value = 0x1000 * self.handles      # (the last argument is byref(handle))
            return 1 if name == "iqd_abi_version" else 0
        setattr(self, name, fn)
        return fn


@pytest.fixture
def lib(monkeypatch):
    rec = capi._bind(Recorder())
    monkeypatch.setattr(capi, "_LIB", rec)
    return rec


def test_the_nine_kinds_are_the_header_s():
    assert sorted(MAKE) == sorted(n[4:-8] for n in capi.PROTOTYPES if n.endswith("_destroy") and n != "iqd_destroy")


@pytest.mark.parametrize("kind", sorted(MAKE))
def test_engine_close_destroys_the_child_first_and_once(lib, kind):
    eng = capi.Engine(1)
    child = MAKE[kind](eng)
    assert lib.calls[-1] == "iqd_%s_create" % kind and child._h.value == 0x2000
    eng.close()
    assert lib.calls[-2:] == ["iqd_%s_destroy" % kind, "iqd_destroy"]
    n = len(lib.calls)
    child.close()
    assert len(lib.calls) == n
    del child
    gc.collect()
    eng.close()
    assert len(lib.calls) == n


@pytest.mark.parametrize("kind", sorted(MAKE))
def test_a_child_that_goes_first_is_destroyed_once(lib, kind):
    eng = capi.Engine(1)
    closed, dropped = MAKE[kind](eng), MAKE[kind](eng)
    closed.close()
    closed.close()
    del dropped
    gc.collect()
    assert lib.calls[-2:] == ["iqd_%s_destroy" % kind] * 2
    eng.close()
    del closed
    gc.collect()
    assert lib.calls.count("iqd_%s_destroy" % kind) == 2 and lib.calls[-1] == "iqd_destroy"


def test_every_child_of_one_engine_goes_before_it(lib):
    eng = capi.Engine(1)
    children = [make(eng) for make in MAKE.values()]
    eng.close()
    assert sorted(lib.calls[-10:-1]) == sorted("iqd_%s_destroy" % k for k in MAKE) and lib.calls[-1] == "iqd_destroy"
    assert not any(c._h for c in children)


def test_a_gatherer_keeps_its_own_error_text(lib, monkeypatch):
    monkeypatch.setattr(lib, "iqd_gather_create", lambda *a: -3)
    monkeypatch.setattr(lib, "iqd_strerror", lambda status: b"status %d" % status)
    eng = capi.Engine(1)
    with pytest.raises(capi.IqdError, match=r"status -3 \(-3\): iqd_gather_create failed \(is librccl.so there\?\)"):
        capi.Gatherer(eng, bytes(128), 0, 1)
    assert "iqd_last_error" not in lib.calls
