"""What the tests of the PCM add-ons (tones, fsk) share: the refusal check of the GPU tier, and the CPU tier's checks of an
add-on's header (include/iqdemod_<kind>.h) against the binding's own prototype table and struct mirrors."""
import os
import re
import subprocess

import pytest

from rtlsdrdiags_amd import capi
from tests.test_abi_layout import mirror_layout
from tests.test_abi_prototypes import C_RETURN, c_param_class, ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def eng():
    """the refusal modules' engine (they import this fixture)"""
    e = capi.Engine(n_channels=1)
    yield e
    e.close()


def refused(eng, fn, *words):
    """fn() raises IQD_EINVAL with every word in its message and queues nothing"""
    before = eng.stats()
    with pytest.raises(capi.IqdError) as err:
        fn()
    assert err.value.status == EINVAL, err.value
    for w in words:
        assert w in str(err.value), (w, str(err.value))
    after = eng.stats()
    assert (after["device_launches"], after["device_copies"]) == (before["device_launches"], before["device_copies"])


def header_path(kind):
    return os.path.join(ROOT, "include", "iqdemod_%s.h" % kind)


def header_text(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def header_prototypes(path):
    """{name: (return class, [parameter classes])} of every function the header declares (the parser of
    tests/test_abi_prototypes.py on this header)"""
    text = "\n".join(l for l in header_text(path).splitlines() if not l.lstrip().startswith("#") and 'extern "C"' not in l)
    text = re.sub(r"\{[^{}]*\}", " ", text)
    out = {}
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        m = re.fullmatch(r"(.*?)\b(iqd_\w+) ?\((.*)\)", stmt)
        if not m:
            assert "(" not in stmt, "a declaration this parser cannot read: %r" % stmt
            continue
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, name
        out[name] = ("pointer" if "*" in ret else C_RETURN[ret.replace("const ", "")],
                     [] if params == "void" else [c_param_class(p.strip()) for p in params.split(",")])
    return out


def check_table_is_header(kind, module, n_functions):
    """the module's PROTOTYPES is the header, function by function and in its order, and shares no name with capi's"""
    header = header_prototypes(header_path(kind))
    assert len(header) == n_functions and list(header) == list(module.PROTOTYPES)
    assert not set(header) & set(capi.PROTOTYPES)
    for name, (ret, params) in header.items():
        restype, argtypes = module.PROTOTYPES[name]
        assert (ctypes_class(restype, returned=True), [ctypes_class(t) for t in argtypes]) == (ret, params), name


def check_library_binding(module):
    """the add-on's library is capi's, with every function of the module's table bound from that table"""
    lib = module._lib()
    assert lib is capi._lib()
    for name, (restype, argtypes) in module.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == list(argtypes), name


def compiled_layouts(kind, mirror, tmp_path):
    """{struct: (size, [(field, offset, size)])} as tests/abi_layout/<kind>_layout_check.c - a stand-alone C program, compiled
    with the address and undefined-behaviour sanitizers - prints them, held against the header's fields and the mirrors"""
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(iqd_\w+)\s*\{(.*?)\}", header_text(header_path(kind)), flags=re.S):
        structs[name] = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert set(structs) == set(mirror)
    exe = str(tmp_path / ("%s_layout_check" % kind))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_layout", "%s_layout_check.c" % kind), "-o", exe],
                   check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, check=True, text=True)
    compiled = {}
    for line in run.stdout.splitlines():
        what, a, b = line.split()
        if what == "struct":
            compiled[a] = (int(b), [])
        else:
            name, field = what.split(".")
            compiled[name][1].append((field, int(a), int(b)))
    assert list(compiled) == list(structs)
    for name, fields in structs.items():
        size, lines = compiled[name]
        assert [f for f, _, _ in lines] == fields, name
        assert mirror_layout(mirror[name]) == (size, lines), name
    return compiled
