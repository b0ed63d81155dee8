"""include/g4d_sets.h, a further header of libg4d_hip.so itself (entry points added after the record of g4d.h, tests/abi_snapshot.txt, was
closed), without a GPU: the header as _lib.parse_header reads it against its record tests/sets_abi_snapshot.txt, the library's exports, the
binding, and the argument checks of the set-form ball query."""
import ctypes
import os
import re

from conftest import ROOT
from test_abi_cpu import _LETTERS

HEADER = os.path.join(ROOT, "include", "g4d_sets.h")
NAME = "g4d_ball_grid_query_set_f32"


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(g4d_[a-z0-9_]+)\s*\(", hdr)))


def test_parsed_sets_header_equals_its_snapshot():
    """Both ways and in the header's order: a changed prototype fails, a new one fails until its line is appended to the record.  The set form
    takes exactly the arguments of the ordered entry point of g4d.h."""
    from garment4d_amd import _lib
    protos, fields, consts = _lib.parse_header(open(HEADER).read())
    parsed = {n: _LETTERS[r] + ":" + "".join(_LETTERS[t] for t in a) for n, (r, a) in protos.items()}
    lines = [ln.split() for ln in open(os.path.join(ROOT, "tests", "sets_abi_snapshot.txt")).read().splitlines()]
    assert all(len(ln) == 2 for ln in lines) and fields == [] and consts == {}
    assert set(parsed) == set(_declared()) and list(parsed) == [ln[0] for ln in lines] and parsed == dict(lines)
    assert protos[NAME] == _lib.PROTOTYPES["g4d_ball_grid_query_f32"]
    assert not set(parsed) & set(_lib.PROTOTYPES)                            # g4d.h's names stay g4d.h's alone


def test_library_exports_the_declared_symbols_and_call_finds_them():
    from garment4d_amd import _lib
    L, protos, _ = _lib.sets_lib()
    for s in _declared():
        fn = getattr(L, s)
        assert list(fn.argtypes) == protos[s][1] and fn.restype is protos[s][0], s
    assert _lib.sets_lib()[0] is L and _lib._entry(NAME) is getattr(L, NAME)
    assert NAME not in _lib.SIGNATURES and _lib.lib().g4d_version() == 263
    assert _lib._entry("g4d_ball_grid_query_f32") is getattr(_lib.lib(), "g4d_ball_grid_query_f32")


def test_argument_validation_needs_no_gpu():
    from garment4d_amd import _lib
    L, _, _ = _lib.sets_lib()
    fn = getattr(L, NAME)
    r, ns = (ctypes.c_float * 2)(0.1, 0.3), (ctypes.c_int * 2)(16, 32)
    out = (ctypes.c_void_p * 2)(8, 8)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    for args, needle in [((-1, 8, 4, 1, p(r), p(ns), 8, 8, p(out), 8, 0.5, None), "bad sizes"),
                         ((1, 8, 4, 5, p(r), p(ns), 8, 8, p(out), 8, 0.5, None), "bad sizes"),
                         ((1, 8, 4, 1, None, p(ns), 8, 8, p(out), 8, 0.5, None), "null pointer"),
                         ((1, 8, 4, 2, p(r), p(ns), 8, 8, p(out), 8, 0.2, None), "exceeds the radius the grid was built for")]:
        assert fn(*args) == 10001, args
        msg = _lib.lib().g4d_last_error().decode()
        assert NAME in msg and needle in msg, msg
    assert fn(0, 8, 4, 1, p(r), p(ns), None, None, p(out), None, 0.5, None) == 0    # empty problems are fine
