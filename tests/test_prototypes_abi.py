"""CPU test of the ctypes prototypes that _lib.load() declares: every name of _lib.C_API + _lib.GPU_API has exactly the restype and the
argtypes recorded in tests/golden/prototypes.json (this module's own output, `python tests/test_prototypes_abi.py`, written before the
prototypes became one table), every vbz_gpu_* entry takes as many arguments as include/vbz_gpu.h declares, and the names that carry a
prototype are the two lists' names, no more and no fewer."""
import ctypes
import json
import os
import re

from test_locate_abi import header, prototype
from vbz_compression_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prototypes.json")
NAMES = _lib.C_API + _lib.GPU_API


def spell(t):
    """a ctypes type as a string: its ctypes name, POINTER(GpuMatch) for a pointer to a struct, None for void"""
    if t is None:
        return "None"
    if issubclass(t, ctypes._Pointer):
        return "POINTER(%s)" % spell(t._type_)
    return t.__name__


def declared(L):
    """name -> [restype, [argtypes]] as strings, of every listed name that load() gave a prototype"""
    out = {}
    for name in NAMES:
        f = getattr(L, name)
        if f.argtypes is not None:
            out[name] = [spell(f.restype), [spell(a) for a in f.argtypes]]
    return out


def header_args(text, name):
    """how many arguments the header declares for `name`"""
    if re.search(r"VBZ_EXPORT\s+int\s+" + name + r"\s*\(", text):
        return len(prototype(text, name))
    # (prototype() reads the entries that return int; create, destroy, the setters and the version string follow the same rule)
    m = re.search(r"VBZ_EXPORT\s+[\w \*]+?\b" + name + r"\s*\((.*?)\);", text, re.S)
    assert m, name
    args = [a.strip() for a in m.group(1).split(",")]
    return 0 if args == ["void"] else len(args)


def test_every_listed_name_has_the_recorded_prototype():
    want = json.load(open(GOLDEN))
    got = declared(_lib.load())
    assert sorted(want) == sorted(NAMES), sorted(set(want) ^ set(NAMES))
    for name in NAMES:
        assert name in got, "%s has no prototype" % name
        assert got[name] == want[name], (name, got[name], want[name])


def test_argument_counts_are_the_headers():
    L, text = _lib.load(), header()
    for name in _lib.GPU_API:
        assert len(getattr(L, name).argtypes) == header_args(text, name), name


def test_the_table_is_the_two_lists():
    want = json.load(open(GOLDEN))
    # (the names that carry a prototype: the module's table where it has one, else what load() set)
    table = getattr(_lib, "PROTOTYPES", None)
    names = list(table) if table is not None else list(declared(_lib.load()))
    assert len(names) == len(set(names))
    assert set(want) <= set(names), sorted(set(want) - set(names))
    assert set(names) <= set(NAMES), sorted(set(names) - set(NAMES))


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(declared(_lib.load()), f, indent=0, sort_keys=True)
        f.write("\n")
