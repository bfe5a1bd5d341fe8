"""Every build switch of the kernel sources is written down where a reader looks for it: the `IQD_*` names that preprocessor
conditionals under rtlsdrdiags_amd/csrc test are exactly those of DESIGN.md 4.9, "Build switches that remain"."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r"IQD_[A-Z0-9_]+")


def switches_in_sources():
    names = set()
    for ext in ("h", "hip", "cpp", "cc"):
        for path in glob.glob(os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "*." + ext)):
            with open(path, encoding="utf-8") as f:
                for line in f:
                    if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                        names.update(NAME.findall(line))
    return names


def switches_in_design():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        text = f.read()
    start = text.index("**Build switches that remain.**")
    items = re.findall(r"^- .*(?:\n  .*)*", text[start:text.index("\n### ", start)], flags=re.M)   # the section's list items
    return set(NAME.findall("\n".join(items)))


def test_every_build_switch_is_listed_in_design():
    src, doc = switches_in_sources(), switches_in_design()
    assert len(doc) > 10, "the list of DESIGN.md 4.9 was not found"
    assert src == doc, "only in the sources: %s; only in DESIGN.md: %s" % (sorted(src - doc), sorted(doc - src))
