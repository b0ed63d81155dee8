"""include/g4d_live.h, the live-cloud scope of libg4d_hip.so (a further header of the library itself, like g4d_sets.h), without a GPU: the
header as _lib.parse_header reads it against its record tests/live_abi_snapshot.txt, the library's exports and the binding; begin / end /
nesting errors; and which launches a scope applies to -- the rule every converted launcher asks (g4d_live_scope_rows_per_cloud)."""
import ctypes
import os
import re
import threading

import pytest

from conftest import ROOT
from test_abi_cpu import _LETTERS

HEADER = os.path.join(ROOT, "include", "g4d_live.h")
EINVAL = 10001


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(g4d_[a-z0-9_]+)\s*\(", hdr)))


@pytest.fixture()
def live():
    """The bound library, with no scope open on this thread before and after the test."""
    from garment4d_amd import _lib
    L, _, _ = _lib.live_lib()
    assert L.g4d_live_scope_capacity() == 0
    yield L
    if L.g4d_live_scope_capacity():
        L.g4d_live_scope_end()


def test_parsed_live_header_equals_its_snapshot():
    """Both ways and in the header's order: a changed prototype fails, a new one fails until its line is appended to the record."""
    from garment4d_amd import _lib
    protos, fields, consts = _lib.parse_header(open(HEADER).read())
    parsed = {n: _LETTERS[r] + ":" + "".join(_LETTERS[t] for t in a) for n, (r, a) in protos.items()}
    lines = [ln.split() for ln in open(os.path.join(ROOT, "tests", "live_abi_snapshot.txt")).read().splitlines()]
    assert all(len(ln) == 2 for ln in lines) and fields == [] and consts == {}
    assert set(parsed) == set(_declared()) and list(parsed) == [ln[0] for ln in lines] and parsed == dict(lines)
    assert not set(parsed) & set(_lib.PROTOTYPES)                            # g4d.h's names stay g4d.h's alone
    assert not set(parsed) & set(_lib.parse_header(open(_lib.SETS_HEADER_PATH).read())[0])


def test_library_exports_the_declared_symbols_and_call_finds_them():
    from garment4d_amd import _lib
    L, protos, _ = _lib.live_lib()
    for s in _declared():
        fn = getattr(L, s)
        assert list(fn.argtypes) == protos[s][1] and fn.restype is protos[s][0], s
        assert s not in _lib.SIGNATURES and _lib._entry(s) is fn
    assert _lib.live_lib()[0] is L and _lib.lib().g4d_version() == 263


def test_begin_end_and_nesting_errors(live):
    from garment4d_amd import _lib
    err = lambda: _lib.lib().g4d_last_error().decode()
    assert live.g4d_live_scope_end() == EINVAL and "no scope is open" in err()
    assert live.g4d_live_scope_begin(None, 4) == EINVAL and "device pointer" in err()
    assert live.g4d_live_scope_begin(64, 0) == EINVAL and live.g4d_live_scope_begin(64, -3) == EINVAL
    assert live.g4d_live_scope_capacity() == 0                               # a refused begin opens nothing
    assert live.g4d_live_scope_begin(64, 4) == 0 and live.g4d_live_scope_capacity() == 4
    assert live.g4d_live_scope_begin(128, 8) == EINVAL and "already open" in err() and "do not nest" in err()
    assert live.g4d_live_scope_capacity() == 4                               # ... and a refused nesting leaves the open one as it is
    assert live.g4d_live_scope_end() == 0 and live.g4d_live_scope_capacity() == 0
    assert live.g4d_live_scope_end() == EINVAL
    assert live.g4d_live_scope_begin(128, 8) == 0 and live.g4d_live_scope_capacity() == 8   # a new scope after the end
    assert live.g4d_live_scope_end() == 0


def test_scope_applies_to_cloud_major_launches_only(live):
    rpc = live.g4d_live_scope_rows_per_cloud
    assert rpc(4, 4096) == 0 and rpc(-1, 4096) == 0                          # no scope: every launch computes everything
    assert live.g4d_live_scope_begin(64, 4) == 0
    assert rpc(4, 4 * 1024) == 1024 and rpc(4, 4 * 17) == 17                 # b == capacity: rows per cloud
    assert rpc(3, 3 * 1024) == 0 and rpc(5, 5 * 1024) == 0 and rpc(8, 8 * 1024) == 0 and rpc(1, 1024) == 0   # b != capacity: ignored
    assert rpc(4, 4 * 1024 + 1) == 0 and rpc(0, 0) == 0 and rpc(4, 0) == 0   # not whole clouds / nothing to launch
    assert rpc(-1, 4 * 96) == 96 and rpc(-1, 4) == 1                         # rows only: a multiple of the capacity
    assert rpc(-1, 4 * 96 + 2) == 0 and rpc(-1, 4 * 96 - 1) == 0 and rpc(-1, 0) == 0 and rpc(-1, -8) == 0
    assert rpc(4, 1 << 31) == 0 and rpc(-1, 1 << 31) == 0                    # (the kernels count rows in 32 bits)
    assert live.g4d_live_scope_end() == 0
    assert rpc(4, 4 * 1024) == 0 and rpc(-1, 4 * 96) == 0                    # closed again


def test_scope_is_per_thread(live):
    seen = {}
    assert live.g4d_live_scope_begin(64, 4) == 0

    def other():
        seen["cap"] = live.g4d_live_scope_capacity()
        seen["rpc"] = live.g4d_live_scope_rows_per_cloud(4, 4096)
        seen["end"] = live.g4d_live_scope_end()                              # nothing of this thread's to end
        seen["begin"] = live.g4d_live_scope_begin(128, 6)                    # ... and room for a scope of its own
        seen["cap2"] = live.g4d_live_scope_capacity()
        live.g4d_live_scope_end()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"cap": 0, "rpc": 0, "end": EINVAL, "begin": 0, "cap2": 6}
    assert live.g4d_live_scope_capacity() == 4 and live.g4d_live_scope_end() == 0


def test_python_context_manager_closes_on_error(live):
    """_lib.live_scope(): begin / end around the block, the end also when the block raises; a refused nesting raises G4DError."""
    from garment4d_amd import _lib

    class FakeCount:   # what live_scope() asks of the count tensor, without a GPU
        is_cuda, dtype = True, "torch.int32"
        numel = staticmethod(lambda: 1)
        data_ptr = staticmethod(lambda: 256)

    with pytest.raises(ZeroDivisionError):
        with _lib.live_scope(FakeCount, 5):
            assert live.g4d_live_scope_capacity() == 5
            with pytest.raises(_lib.G4DError, match="do not nest"):
                with _lib.live_scope(FakeCount, 5):
                    pass
            assert live.g4d_live_scope_capacity() == 5
            1 / 0
    assert live.g4d_live_scope_capacity() == 0
