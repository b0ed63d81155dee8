"""CPU-side checks of how garment4d_amd/_lib.py reads a header and marshals host data: the parser on a short synthetic header with every
form include/g4d.h uses, the host-array and workspace helpers, and the lines G4D_TRACE_CALLS prints (texts recorded from the binding as it
was with hand-typed tables)."""
import ctypes

import pytest

from garment4d_amd import _lib

HEADER = """
/* a comment with a prototype inside: int g4d_ghost(int a, float *b); and (parentheses) */
#ifndef X_H
#define X_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct ihipStream_t *g4d_stream_t; /* == hipStream_t */
#define G4D_OK 0
#define G4D_EINVAL 10001 /* bad argument (negative size) */
#define G4D_NOT_A_NUMBER something
int g4d_version(void); /* 100 * major + minor (entry points added, none changed: g4d_ghost2(int)) */
const char *g4d_last_error(void);
int g4d_many_f32(int b, long long rows, float radius, const float *xyz, float *out,
                 const float *const *scale, int *const *idx,
                 float *const *dst, const void *grid, const unsigned short *const *W,
                 g4d_stream_t stream);
long long g4d_ws_bytes(long long rows, int c);
size_t g4d_scratch_floats(int n);
unsigned g4d_args_size(void);
int g4d_set(const char *name, long long value);
enum g4d_mlp_family {
    G4D_MLP_A = 0,   /* g4d_a: (x) */
    G4D_MLP_B = 1,
    G4D_MLP_C = 2 /* last */
};
typedef struct g4d_mlp_args {
    unsigned size, version;
    long long rows;                /* rows (all of them) */
    const float *X; int ldx;
    const float *xyz, *new_xyz; const int *idx;
    const void *const *W;
    const float *const *scale, *const *shift;
    float *out; int ldo, col0;
} g4d_mlp_args;
int g4d_run(int family, const g4d_mlp_args *args, g4d_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""

I, F, Q, Z, U, P, S = (ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_char_p)


def test_parser_reads_every_form_the_header_uses():
    protos, fields, consts = _lib.parse_header(HEADER)
    assert protos == {
        "g4d_version": (I, []),
        "g4d_last_error": (S, []),
        "g4d_many_f32": (I, [I, Q, F, P, P, P, P, P, P, P, P]),     # spans four lines; every pointer form and g4d_stream_t -> c_void_p
        "g4d_ws_bytes": (Q, [Q, I]),
        "g4d_scratch_floats": (Z, [I]),
        "g4d_args_size": (U, []),
        "g4d_set": (I, [S, Q]),
        "g4d_run": (I, [I, P, P]),
    }
    assert "g4d_ghost" not in protos and "g4d_ghost2" not in protos          # prototypes inside comments are no prototypes
    assert fields == [("size", U), ("version", U), ("rows", Q), ("X", P), ("ldx", I), ("xyz", P), ("new_xyz", P), ("idx", P), ("W", P),
                      ("scale", P), ("shift", P), ("out", P), ("ldo", I), ("col0", I)]
    assert consts == {"G4D_OK": 0, "G4D_EINVAL": 10001, "G4D_MLP_A": 0, "G4D_MLP_B": 1, "G4D_MLP_C": 2}


@pytest.mark.parametrize("decl, name", [
    ("int g4d_odd_f32(int b, double x);", "g4d_odd_f32"),                  # a scalar the map does not know
    ("int g4d_odd2_f32(int b, short);", "g4d_odd2_f32"),                   # unnamed: nothing is guessed
    ("double g4d_odd3(void);", "g4d_odd3"),                                # ... as a return type
])
def test_parser_refuses_an_unknown_type_by_name(decl, name):
    with pytest.raises(_lib.G4DError, match=name):
        _lib.parse_header(HEADER + decl)


def test_parser_refuses_a_statement_it_cannot_read():
    with pytest.raises(_lib.G4DError, match="callback"):
        _lib.parse_header(HEADER + "int g4d_cb(int (*callback)(int));")


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4097])
def test_workspace_never_rounds_down(n):
    import torch
    ws = _lib.workspace(n, torch.device("cpu"))
    assert ws.dtype == torch.uint8 and ws.numel() == max(n, 16) and ws.device.type == "cpu"


def test_host_array_round_trips():
    ints = _lib.host_array(ctypes.c_int, [3, -1, 2 ** 31 - 1])
    assert isinstance(ints, ctypes.c_void_p) and list(ctypes.cast(ints, ctypes.POINTER(ctypes.c_int))[:3]) == [3, -1, 2 ** 31 - 1]
    floats = _lib.host_array(ctypes.c_float, [0.25, -1.5])
    assert list(ctypes.cast(floats, ctypes.POINTER(ctypes.c_float))[:2]) == [0.25, -1.5]
    ptrs = _lib.host_array(ctypes.c_void_p, [0, 4096, 2 ** 47 + 8])
    assert list(ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))[:3]) == [None, 4096, 2 ** 47 + 8]
    wide = _lib.host_array(ctypes.c_longlong, [2 ** 40])
    assert ctypes.cast(wide, ctypes.POINTER(ctypes.c_longlong))[0] == 2 ** 40


def test_trace_lines(monkeypatch, capfd):
    """G4D_TRACE_CALLS: a g4d_mlp_run names the kernel family behind its argument block and the block's fifteen leading integers, then goes
    on like any call, which prints its int and float arguments.  rows = 0: validated and returned without a launch, so no GPU is needed."""
    _lib.lib()
    monkeypatch.setattr(_lib, "_TRACE", True)
    a = _lib.MlpArgs(mode=0, rows=0, K0=3, ldx=3, N=5, P=6, S=7, C=8, use_xyz=1, n=9, m=10, C2=11, C1=12, nlayers=2, pool=1)
    shown = "0 0 3 3 5 6 7 8 1 9 10 11 12 2 1"
    assert _lib.call("g4d_mlp_run", _lib.MLP_CHAIN_F32, ctypes.pointer(a), None) == 0
    assert capfd.readouterr().err == f"g4d call g4d_mlp_run -> g4d_mlp_chain_f32 {shown}\ng4d call g4d_mlp_run 3\n"
    assert _lib.call("g4d_mlp_run", _lib.MLP_STACK_BF16, ctypes.pointer(a), None) == 0
    assert capfd.readouterr().err == f"g4d call g4d_mlp_run -> g4d_mlp_stack_bf16 {shown}\ng4d call g4d_mlp_run 1\n"
    assert _lib.call("g4d_mlp_run", _lib.MLP_WAVE_F32, ctypes.addressof(a), 0) == 0          # the block by address, stream 0 as an int
    assert capfd.readouterr().err == f"g4d call g4d_mlp_run -> g4d_mlp_wave_f32 {shown}\ng4d call g4d_mlp_run 2 0\n"
    a.unknown_grid = 4096
    assert _lib.call("g4d_mlp_run", _lib.MLP_CHAIN_BF16, ctypes.pointer(a), None) == 0
    assert capfd.readouterr().err == f"g4d call g4d_mlp_run -> g4d_mlp_chain_cells_bf16 {shown}\ng4d call g4d_mlp_run 4\n"
    assert _lib.call("g4d_fps_f32", 0, 8, 4, 0, 0, 0, 0) == 0
    assert capfd.readouterr().err == "g4d call g4d_fps_f32 0 8 4 0 0 0 0\n"
    assert _lib.call("g4d_ball_query_f32", 0, 8, 4, 0.25, 4, None, None, None, None) == 0
    assert capfd.readouterr().err == "g4d call g4d_ball_query_f32 0 8 4 0.25 4\n"
    monkeypatch.setattr(_lib, "_TRACE", False)
    assert _lib.call("g4d_fps_f32", 0, 8, 4, 0, 0, 0, 0) == 0 and capfd.readouterr().err == ""
