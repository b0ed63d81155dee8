"""The exact-arithmetic cases of tests/test_bf16_exact_gpu.py, checked on the CPU before anything is sent to a GPU: every case is inside the exact
regime and exercises the roundings (bf16_exact_twin.check_conditions), and the float64 twin is SENSITIVE -- each deliberate fault (truncation
instead of round-to-nearest-even, ties away from zero, a dropped last input column, two columns of one k-step swapped, a pool window shifted by
one row) changes the expected output of every case it applies to, so a kernel with that fault could not pass the GPU comparison.  One test keeps
the Python list of bf16 chain tiles in step with the case labels of the switch in csrc/mlp_chain_bf16.hip."""
import os
import re

import pytest
import torch

import bf16_exact_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = [(g, c) for g, cs in (("stack", T.STACK_CASES), ("sa", T.SA_CASES), ("fp_head", T.FP_HEAD_CASES), ("gemm", T.GEMM_CASES), ("module", T.MODULE_CASES))
         for c in cs]
IDS = [f"{g}:{c['id']}" for g, c in EVERY]


@pytest.mark.parametrize("case", [c for _, c in EVERY], ids=IDS)
def test_conditions_hold(case):
    for precision in case["precisions"]:
        inp, stack = T.build(case, precision)
        T.check_conditions(inp, stack, precision, pool=case["pool"], S=case["S"])


def _differs(case, precision, **mut):
    inp, stack = T.build(case, precision)
    ref, ref_tap = T.want(case, precision)
    out, tap = T.expected(inp, stack, precision, pool=case["pool"], S=case["S"], tap=case["tap"], **mut)
    return not torch.equal(out, ref) or (tap is not None and not torch.equal(tap, ref_tap))     # (the GPU tests compare both)


@pytest.mark.parametrize("case", [c for _, c in EVERY], ids=IDS)
def test_twin_notices_each_fault(case):
    assert "bf16" in case["precisions"]
    for rule in ("trunc", "away"):                       # the roundings exist in "bf16" only
        assert _differs(case, "bf16", mut=rule), f"{rule} instead of round-to-nearest-even goes unnoticed"
    for precision in dict.fromkeys("bf16" if p == "bf16" else "fp32" for p in case["precisions"]):   # "bf16x3" has the twin of "fp32"
        for l in range(len(case["widths"]) - 1):
            for m in ("drop_last_col", "swap_cols"):
                assert _differs(case, precision, mut=m, mut_layer=l), f"{m} at layer {l} goes unnoticed ({precision})"
        if case["pool"]:
            assert _differs(case, precision, mut="pool_shift"), f"a pool window shifted by one row goes unnoticed ({precision})"


def test_rounding_rules_differ_only_where_they_should():
    x = T.lattice_values((4096,), T._gen(3))
    rne, away, trunc = (T.round_bf16(x, r) for r in ("rne", "away", "trunc"))
    tie = T.is_tie(x)
    assert torch.equal(rne[~tie], away[~tie]) and bool((rne[tie] != away[tie]).any()) and bool((rne[tie] == away[tie]).any())
    assert torch.equal(trunc[~T.not_bf16(x)], x[~T.not_bf16(x)]) and bool((trunc.abs() <= x.abs()).all())
    one = torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875], dtype=T.F64)     # 1 + 2^-8 (even below), 1 + 3 * 2^-8 (odd below)
    assert T.round_bf16(one).tolist() == [1.0, 1.015625, -1.0, -1.015625]
    assert T.round_bf16(one, "away").tolist() == [1.0078125, 1.015625, -1.0078125, -1.015625]
    assert T.round_bf16(one, "trunc").tolist() == [1.0, 1.0078125, -1.0, -1.0078125]


def _switch_tiles(path, impl):
    src = open(os.path.join(ROOT, "garment4d_amd", "csrc", path)).read()
    body = src[src.index(impl):]
    body = body[body.index("switch (key)"):body.index("#undef G4D_CHAIN")]
    body = body.split("#else")[-1]                       # (the fp32 file keeps a short list for development builds in front)
    keys = [int(k) for k in re.findall(r"case (\d+): G4D_CHAIN", body)]
    assert "default: G4D_REQUIRE(false" in body, "the switch must refuse unlisted widths before any launch"
    return {tuple(t for t in (k // 1000000, k // 10000 % 100, k // 100 % 100, k % 100) if t) for k in keys}


def test_bf16_tile_list_matches_the_switch():
    from garment4d_amd import fused
    bf16 = _switch_tiles("mlp_chain_bf16.hip", "static int chain_bf16_impl")
    assert bf16 == fused._CHAIN_TILES_BF16 == T.BF16_SWITCH_TILES
    fp32 = _switch_tiles("mlp_chain.hip", "static int chain_launch_one")
    assert fp32 == fused._CHAIN_TILES and fp32 - bf16 == T.FP32_ONLY_TILES
    ran = {T.tiles(c["widths"]) for c in T.STACK_CASES}
    assert bf16 | T.FP32_ONLY_TILES <= ran, "a case label of either switch without an exact-arithmetic case"
    assert any(t not in fp32 for t in ran), "no case for the LDS stack kernel"


def test_raw_bf16_entry_refuses_widths_without_an_instantiation():
    """The switch of chain_bf16_impl has no case for 32-64 (g4d_mlp_chain_supported lists it for the fp32 kernel): the entry point fails with its
    own message before any launch -- so this runs without a GPU (no pointer below is dereferenced on the host beyond the per-layer arrays)."""
    import ctypes
    from garment4d_amd import _lib, fused
    layers = [fused.PackedLayer(W.float(), sc.float(), sh.float(), relu=relu) for W, sc, sh, relu in T.make_stack((32, 32, 64), 1)]
    X, out = torch.zeros(64, 32), torch.zeros(64, 64)
    n = len(layers)
    PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    W, Sc, Sh = PA(*[L.Wc16.data_ptr() for L in layers]), PA(*[L.scale.data_ptr() for L in layers]), PA(*[L.shift.data_ptr() for L in layers])
    W3 = (ctypes.c_void_p * (3 * n))(*[t.data_ptr() for L in layers for t in L.Wc16x3()])
    Kp, Co, Re = IA(*[L.Kpad for L in layers]), IA(*[L.Cout for L in layers]), IA(*[L.relu for L in layers])
    for entry, w in (("g4d_mlp_chain_bf16", W), ("g4d_mlp_chain_bf16x3", W3)):
        with pytest.raises(_lib.G4DError, match="no bf16 instantiation"):
            _lib.call(entry, 0, 64, 32, X.data_ptr(), 32,                      # mode (direct), rows, K0, X, ldx
                      0, 0, 1, 0, 0, 0, 0, 0, 0,                               # N, P, S, C, use_xyz, xyz, new_xyz, feats, idx
                      0, 0, 0, 0, 0, 0, 0, 0,                                  # n, m, C2, C1, known_feats, skip, dist2, nn_idx
                      n, vp(w), vp(Sc), vp(Sh), vp(Kp), vp(Co), vp(Re), 0, out.data_ptr(), 64, 0, -1, 0, 0, 0)
