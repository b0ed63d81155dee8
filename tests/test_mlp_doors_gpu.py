"""Both doors of the whole-stack MLP launchers launch the same thing: for each of the seven kernel families and each loader, the same inputs go
through the positional entry point and through g4d_mlp_run into sentinel-filled outputs, and the two results -- the output window, the columns
outside it, the tapped layer -- must be torch.equal.  The shapes are the smallest that keep every argument apart from its neighbours (two clouds,
N != P * S, n != m, ldx > K0, an output window inside a wider tensor), so a transposed argument in one adapter shows.  Where the exact twin
(tests/bf16_exact_twin.py) covers the loader, the window is also compared with it."""
import ctypes

import pytest
import torch

import bf16_exact_twin as T
import mlp_doors as D
from garment4d_amd import _lib, fused, synthetic as syn
from mlp_doors import SENTINEL, dev, packed, same

pytestmark = pytest.mark.gpu

WIDTHS = (32, 32, 64)      # every family instantiates 32-32-64 (both tile sets of the twin list it)
COL0, LDO = 8, 8 + 64 + 8
PRECISION = {"stack_f32": "fp32", "wave_f32": "fp32", "chain_f32": "fp32", "stack_bf16": "bf16", "chain_bf16": "bf16", "chain_cells_bf16": "bf16",
             "chain_bf16x3": "bf16x3"}
WEIGHT = {"stack_f32": "Wf", "wave_f32": "Wf", "chain_f32": "Wf", "stack_bf16": "Wf16", "chain_bf16": "Wc16", "chain_cells_bf16": "Wc16"}

_SHARED, _WANT = {}, {}


def want(kind, precision, inp, stack, pool, S, tap):
    """The twin's (output, tapped layer) of a loader's case, inside its exact regime: computed once per precision, read-only."""
    if (kind, precision) not in _WANT:
        T.check_conditions(inp, stack, precision, pool=pool, S=S)
        _WANT[kind, precision] = T.expected(inp, stack, precision, pool=pool, S=S, tap=tap)
    return _WANT[kind, precision]


def loader(kind):
    """(twin inputs | None, stack, loader fields of the call, pool, S, output rows) -- built once per loader and shared (read-only)."""
    if kind in _SHARED:
        return _SHARED[kind]
    if kind == "direct":
        inp = T.make_inputs("direct", 11, rows=64, K0=32)
        X = torch.full((64, 40), SENTINEL, device="cuda")       # ldx = 40 > K0 = 32
        X[:, :32] = dev(inp["X"])
        f, keep, pool, S, orows = dict(mode=0, rows=64, K0=32, X=X.data_ptr(), ldx=40), [X], 0, 0, 64
    elif kind == "group":
        inp = T.make_inputs("group", 12, B=2, N=32, P=2, S=16, C=13)
        keep = [dev(inp["xyz"]), dev(inp["new_xyz"]), dev(inp["feats"]), inp["idx"].cuda().contiguous()]
        f = dict(mode=1, rows=64, K0=16, N=32, P=2, S=16, C=13, use_xyz=1, xyz=keep[0].data_ptr(), new_xyz=keep[1].data_ptr(), feats=keep[2].data_ptr(),
                 idx=keep[3].data_ptr())
        pool, S, orows = 1, 16, 4
    elif kind == "interp":
        inp = T.make_inputs("interp", 13, B=2, n=32, m=8, C2=16, C1=16, frac=6)    # (interpolation adds two lattice bits)
        keep = [dev(inp["known"]), dev(inp["skip"]), dev(inp["dist2"]), inp["nn_idx"].cuda().contiguous()]
        f = dict(mode=2, rows=64, K0=32, n=32, m=8, C2=16, C1=16, known_feats=keep[0].data_ptr(), skip=keep[1].data_ptr(), dist2=keep[2].data_ptr(),
                 nn_idx=keep[3].data_ptr())
        pool, S, orows = 0, 0, 64
    else:   # two frames of a 32-vertex ring: row v aggregates 0.5 v + 0.25 (v - 1) + 0.25 (v + 1)
        inp = None
        X = dev(T.make_inputs("direct", 14, rows=64, K0=32)["X"])
        v = torch.arange(32)
        rowptr = (3 * torch.arange(33)).int().cuda()
        colidx = torch.stack([v, (v - 1) % 32, (v + 1) % 32], 1).reshape(-1).int().cuda()
        vals = torch.tensor([0.5, 0.25, 0.25]).repeat(32).cuda()
        keep = [X, rowptr, colidx, vals]
        f = dict(mode=3, rows=64, K0=32, X=X.data_ptr(), ldx=32, Vg=32, rowptr=rowptr.data_ptr(), colidx=colidx.data_ptr(), vals=vals.data_ptr())
        pool, S, orows = 0, 0, 64
    stack = T.make_stack((f["K0"],) + WIDTHS, 100 + len(kind), nnz=T.NNZ, probe=None if inp is None else T.layer0_rows(inp))
    _SHARED[kind] = (inp, stack, packed(stack), f, keep, pool, S, orows)
    return _SHARED[kind]


RUNS = [(fam, kind) for fam in D.FAMILIES for kind in ("direct", "group", "interp", "csr") if kind != "csr" or fam in ("stack_f32", "stack_bf16", "wave_f32")]


@pytest.mark.parametrize("family,kind", RUNS, ids=[f"{f}-{k}" for f, k in RUNS])
def test_positional_entry_and_argument_block_launch_the_same(family, kind):
    inp, stack, layers, loader_fields, _keep, pool, S, orows = loader(kind)
    arrays = list(fused.layer_arrays(layers, WEIGHT.get(family, "Wf")))
    if family == "chain_bf16x3":
        arrays[0] = _lib.host_array(ctypes.c_void_p, [t.data_ptr() for L in layers for t in L.Wc16x3()])
    tapped = kind == "interp" and family != "wave_f32"      # a tap on layer 0 (the wave kernel has none)
    grid = None
    if family == "chain_cells_bf16":     # (at this size the persistent kernel declines: the launch is the chain kernel's, through the cells adapter)
        unknown = torch.from_numpy(syn.unit_cloud(2, 32, seed=32)).cuda()
        grid = fused.build_ball_grid(unknown, 0.1)[0]
    results = []
    for door in (D.positional, D.run):
        out = torch.full((orows, LDO), SENTINEL, device="cuda")
        tap = torch.full((64, WIDTHS[0] + 8), SENTINEL, device="cuda")
        f = dict(loader_fields, nlayers=3, pool=pool, S=S, out=out.data_ptr(), ldo=LDO, col0=COL0,
                 **dict(zip(("W", "scale", "shift", "Kpad", "Cout", "relu"), arrays)))
        if tapped:
            f.update(tap_layer=0, tap_out=tap.data_ptr(), tap_ld=tap.shape[1])
        if grid is not None:
            f["unknown_grid"] = grid.data_ptr()
        assert door(family, f, _lib.stream_ptr()) == (0, "")
        torch.cuda.synchronize()
        results.append((out, tap))
    (out_p, tap_p), (out_b, tap_b) = results
    assert torch.equal(out_p, out_b) and torch.equal(tap_p, tap_b)
    window = out_p[:, COL0:COL0 + WIDTHS[-1]]
    assert bool((window != SENTINEL).all()), "the launch did not fill its output window"
    assert bool((out_p[:, :COL0] == SENTINEL).all()) and bool((out_p[:, COL0 + WIDTHS[-1]:] == SENTINEL).all()), "columns outside the output window were written"
    assert bool((tap_p[:, WIDTHS[0]:] == SENTINEL).all()) and bool((tap_p[:, :WIDTHS[0]] != SENTINEL).all()) == tapped
    if inp is not None:
        want_out, want_tap = want(kind, PRECISION[family], inp, stack, pool, max(S, 1), 0 if kind == "interp" else None)
        same(window, want_out, f"{family} / {kind}")
        if tapped:
            same(tap_p[:, :WIDTHS[0]], want_tap, f"{family} / {kind}: tapped layer 0")
