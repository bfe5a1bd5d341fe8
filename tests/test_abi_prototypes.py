"""CPU tier: the binding's prototype table (rtlsdrdiags_amd/capi.py: PROTOTYPES) against include/iqdemod.h, function by
function - the same set of names, the same number of parameters, every parameter and the return value of the same class.
ctypes takes a call of a function without a prototype as it comes and cuts a Python integer to a C int, so a function the
table misses, or a 64-bit parameter it declares as 32 bits, would lose the upper half of an address or a count without a
word.  Reads the header and the table only: no library, no GPU."""
import ctypes as C
import glob
import inspect
import os
import re
import types

from rtlsdrdiags_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PARAM = {"float": "float", "double": "double",
           "uint64_t": "i64", "int64_t": "i64", "size_t": "i64", "unsigned long long": "i64",
           "int": "i32", "uint32_t": "i32", "int32_t": "i32"}
C_RETURN = {"void": "none", "uint64_t": "64", "int64_t": "64", "size_t": "64", "unsigned long long": "64",
            "int": "s32", "int32_t": "s32", "uint32_t": "u32"}


def header_prototypes():
    """{name: (return class, [parameter classes])} of every function the header declares"""
    text = open(os.path.join(ROOT, "include", "iqdemod.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)                        # comments (some run over #define lines) ...
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#") and 'extern "C"' not in l)   # ... # lines
    text = re.sub(r"\{[^{}]*\}", " ", text)                                   # struct and enum bodies
    out = {}
    for stmt in (" ".join(s.split()) for s in text.split(";")):              # (a prototype over several lines is one statement)
        m = re.fullmatch(r"(.*?)\b(iqd_\w+) ?\((.*)\)", stmt)
        if not m:
            assert "(" not in stmt, "a declaration this parser cannot read: %r" % stmt
            continue
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, name
        out[name] = ("pointer" if "*" in ret else C_RETURN[ret.replace("const ", "")],
                     [] if params == "void" else [c_param_class(p.strip()) for p in params.split(",")])
    return out


def c_param_class(p):
    if "*" in p or re.search(r"\[\d*\]$", p):
        return "pointer"
    words = [w for w in p.split() if w != "const"]
    kind = " ".join(words) if " ".join(words) in C_PARAM else " ".join(words[:-1])     # (with or without the parameter's name)
    return C_PARAM[kind]                                                      # an unknown type name is a KeyError: a failure


def ctypes_class(t, returned=False):
    if t is None:
        assert returned
        return "none"
    if issubclass(t, C._Pointer) or t in (C.c_void_p, C.c_char_p):
        return "pointer"
    if t in (C.c_float, C.c_double):
        return "float" if t is C.c_float else "double"
    code, size = t._type_, C.sizeof(t)
    assert issubclass(t, C._SimpleCData) and code in "ilqILQ" and size in (4, 8), t
    if not returned:
        return "i%d" % (8 * size)
    return "64" if size == 8 else ("s32" if code.islower() else "u32")


def test_the_table_is_the_header():
    header = header_prototypes()
    assert len(header) == 121
    assert set(header) == set(capi.PROTOTYPES), sorted(set(header) ^ set(capi.PROTOTYPES))
    assert capi.EXPORTS == list(capi.PROTOTYPES)
    wrong = []
    for name, (ret, params) in header.items():
        restype, argtypes = capi.PROTOTYPES[name]
        mine = (ctypes_class(restype, returned=True), [ctypes_class(t) for t in argtypes])
        if mine != (ret, params):
            wrong.append((name, "header", (ret, params), "table", mine))
    assert not wrong, wrong


def test_the_classifiers_know_their_classes():
    """the parser on declarations of every class, among them the forms the header uses once"""
    assert c_param_class("int16_t out[8192]") == "pointer" and c_param_class("const size_t *bytes_per_rank") == "pointer"
    assert c_param_class("unsigned long long n") == "i64" and c_param_class("uint64_t") == "i64"
    assert c_param_class("const float gain") == "float" and c_param_class("int32_t dbfs") == "i32"
    assert ctypes_class(C.c_size_t) == "i64" and ctypes_class(C.c_int) == "i32" and ctypes_class(C.c_uint32, True) == "u32"
    assert ctypes_class(C.POINTER(capi.Stats)) == "pointer" and ctypes_class(C.c_char_p, True) == "pointer"
    try:
        c_param_class("long n")
    except KeyError:
        pass
    else:
        raise AssertionError("an unknown type name must fail")


def test_every_prototype_is_set_at_load_and_nowhere_else():
    """_bind, what _lib() hands the loaded library to, gives all 121 functions their prototype; no other line of the package
    assigns one."""
    stub = types.SimpleNamespace(**{name: types.SimpleNamespace() for name in capi.PROTOTYPES})
    assert capi._bind(stub) is stub
    for name, (restype, argtypes) in capi.PROTOTYPES.items():
        fn = getattr(stub, name)
        assert fn.restype is restype and fn.argtypes == list(argtypes), name
    lines = [l for f in glob.glob(os.path.join(ROOT, "rtlsdrdiags_amd", "*.py")) for l in open(f) if re.search(r"argtypes|restype", l)]
    loop = inspect.getsource(capi._bind).splitlines(keepends=True)
    assert lines and all(l in loop for l in lines), lines
    assert sum(".argtypes" in l for l in lines) == 1 and sum(".restype" in l for l in lines) == 1, lines
