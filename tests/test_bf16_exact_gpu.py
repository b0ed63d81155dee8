"""The bf16-operand kernels (csrc/mlp_chain_bf16.hip, mlp_stack_bf16.hip, sa_group_bf16.hip, fp_head_bf16.hip, gemm_bf16.hip), bit for bit.

Their other tests allow a few percent of the tensor scale (two correct bf16 pipelines differ wherever a hidden activation lands on the other
side of a rounding boundary) or compare one bf16 kernel with another.  Here the inputs sit on a dyadic lattice on which every product and every
partial sum is exact in fp32 (tests/bf16_exact_twin.py): the only roundings left are the operand conversions to bf16, round-to-nearest-even
decides each of them, and the float64 twin gives the expected output EXACTLY -- every comparison is torch.equal.  tests/test_bf16_exact_cpu.py
proves on the CPU that truncation, a wrong tie rule, a dropped tail column, two swapped columns of a k-step or a pool window off by one row
would change the expected output of every case.  "fp32" and "bf16x3" run the same cases where a chain kernel takes them: nothing rounds there."""
import ctypes

import pytest
import torch

import bf16_exact_twin as T
from garment4d_amd import _lib, fused, pointnet2_modules as PM, pytorch_utils as pt_utils, synthetic as syn, tuning as TU

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def dev(t, dtype=torch.float32):
    if t is None:
        return None
    if dtype == torch.float32:
        assert torch.equal(t.to(torch.float32).to(T.F64), t)
    return t.to(dtype).cuda().contiguous()


def native(**kv):
    return TU.use(TU.current().replace(native=kv))


def packed(stack):
    return [fused.PackedLayer(dev(W), dev(sc), dev(sh), relu=relu) for W, sc, sh, relu in stack]


def same(got, want, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} values differ from the exact twin, first at {bad.nonzero()[0].tolist()}: " \
                                f"{got[bad][0].item()!r} for {want[bad][0].item()!r}"


def family(precision, widths, cells=False):
    t = T.tiles(widths)
    if precision == "bf16":
        return ("g4d_mlp_chain_cells_bf16" if cells else "g4d_mlp_chain_bf16") if t in T.BF16_SWITCH_TILES else "g4d_mlp_stack_bf16"
    if precision == "bf16x3" and t in T.BF16_SWITCH_TILES:
        return "g4d_mlp_chain_bf16x3"
    assert t in T.BF16_SWITCH_TILES | T.FP32_ONLY_TILES
    return "g4d_mlp_chain_f32"


def loader_args(inp):
    """(mode, keyword arguments of fused.mlp_stack) for a case's inputs."""
    if inp["kind"] == "direct":
        X = dev(inp["X"])
        return 0, dict(X=X, ldx=X.shape[1])
    if inp["kind"] == "group":
        return 1, dict(group=(inp["N"], inp["P"], inp["C"], 1, dev(inp["xyz"]), dev(inp["new_xyz"]), dev(inp["feats"]), inp["idx"].cuda().contiguous()))
    return 2, dict(interp=(inp["n"], inp["m"], inp["C2"], inp["C1"], dev(inp["known"]), dev(inp["skip"]), dev(inp["dist2"]), inp["nn_idx"].cuda().contiguous()))


def run_stack(case, precision, cells=False):
    inp, stack = T.build(case, precision)
    layers = packed(stack)
    mode, kw = loader_args(inp)
    rows, cout = inp["rows"], case["widths"][-1]
    orow = rows // case["S"] if case["pool"] else rows
    col0, extra = case["window"] or (0, 0)
    out = torch.full((orow, col0 + cout + extra), SENTINEL, device="cuda")
    tap = None
    if case["tap"] is not None:
        tap = (case["tap"], torch.full((rows, case["widths"][case["tap"] + 1]), SENTINEL, device="cuda"))
    if cells:
        unknown = torch.from_numpy(syn.unit_cloud(inp["B"], inp["n"], seed=inp["n"])).cuda()
        kw["cells_grid"] = fused.build_ball_grid(unknown, 0.1)[0]
    with torch.no_grad(), fused.precision(precision), _lib.timed_calls() as t:
        fused.mlp_stack(mode, rows, inp["K0"], layers, out, col0=col0, pool=case["pool"], S=case["S"], tap=tap, **kw)
    names = [r[0] for r in t.results() if r[0].startswith("g4d_mlp_")]
    assert names == [family(precision, case["widths"], cells)], names
    want, want_tap = T.want(case, precision)
    same(out[:, col0:col0 + cout], want, f"{case['id']} ({precision})")
    assert bool((out[:, :col0] == SENTINEL).all()) and bool((out[:, col0 + cout:] == SENTINEL).all()), "columns outside the output window were written"
    if tap is not None:
        same(tap[1], want_tap, f"{case['id']} ({precision}): tapped layer {case['tap']}")


STACK_RUNS = [(c, p) for c in T.STACK_CASES for p in c["precisions"]]


@pytest.mark.parametrize("case,precision", STACK_RUNS, ids=[f"{c['id']}-{p}" for c, p in STACK_RUNS])
def test_mlp_stack_is_exact(case, precision):
    """fused.mlp_stack on the register-chain kernels (bf16, bf16x3, fp32) and the LDS stack kernel (bf16) against the exact twin."""
    run_stack(case, precision)


@pytest.mark.parametrize("case", [c for c in T.STACK_CASES if c["kind"] == "interp" and T.tiles(c["widths"]) in T.BF16_SWITCH_TILES], ids=lambda c: c["id"])
def test_cell_ordered_interpolating_launch_is_exact(case):
    """g4d_mlp_chain_cells_bf16: the interpolating chain cases again with the unknown cloud's ball grid -- the same expected rows in the same positions."""
    run_stack(case, "bf16", cells=True)


def test_raw_bf16_entry_refuses_widths_without_an_instantiation():
    """32-64 (key 2040000) passes g4d_mlp_chain_supported -- the fp32 kernel has it -- but the bf16 switch has no case for it: the entry point
    must fail before any launch (it used to run the four-layer instantiation on two zero-initialised layers)."""
    X = torch.zeros(64, 32, device="cuda")
    out = torch.full((64, 64), SENTINEL, device="cuda")
    layers = packed(T.make_stack((32, 32, 64), 1))
    n = len(layers)
    PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    W, Sc, Sh = PA(*[L.Wc16.data_ptr() for L in layers]), PA(*[L.scale.data_ptr() for L in layers]), PA(*[L.shift.data_ptr() for L in layers])
    Kp, Co, Re = IA(*[L.Kpad for L in layers]), IA(*[L.Cout for L in layers]), IA(*[L.relu for L in layers])
    with pytest.raises(_lib.G4DError, match="no bf16 instantiation"):
        _lib.call("g4d_mlp_chain_bf16", 0, 64, 32, X.data_ptr(), 32,          # mode (direct), rows, K0, X, ldx
                  0, 0, 1, 0, 0, 0, 0, 0, 0,                                   # N, P, S, C, use_xyz, xyz, new_xyz, feats, idx
                  0, 0, 0, 0, 0, 0, 0, 0,                                      # n, m, C2, C1, known_feats, skip, dist2, nn_idx
                  n, vp(W), vp(Sc), vp(Sh), vp(Kp), vp(Co), vp(Re), 0, out.data_ptr(), 64, 0, -1, 0, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- modules
def load_blocks(blocks, stack):
    """The lattice stack into conv blocks without BatchNorm: W as the conv weight, the shift as the conv bias (_fold then gives scale 1 exactly)."""
    blocks = [b for b in blocks if not isinstance(b, torch.nn.Dropout)]
    assert len(blocks) == len(stack)
    with torch.no_grad():
        for b, (W, scale, shift, relu) in zip(blocks, stack):
            assert bool((scale == 1).all()) and (getattr(b, "activation", None) is not None) == relu
            b.conv.weight.copy_(W.float().view(b.conv.weight.shape))
            b.conv.bias.copy_(shift.float())


def sa_module(case, stack):
    sh = case["shape"]
    sa = PM.PointnetSAModule(npoint=sh["P"], radius=1.0, nsample=sh["S"], mlp=[sh["C"]] + list(case["widths"][1:]), bn=False)
    load_blocks(list(sa.mlps[0].children()), stack)
    return sa.cuda().eval()


def run_sa(case, precision, expect_family, **native_kv):
    inp, stack = T.build(case, precision)
    sa = sa_module(case, stack)
    rep = case.get("rep", 1)
    grow = lambda t: None if t is None else (t.expand(rep, *t.shape[1:]).contiguous() if rep > 1 else t)
    xyz, new_xyz, feats, idx = grow(dev(inp["xyz"])), grow(dev(inp["new_xyz"])), grow(dev(inp["feats"])), grow(inp["idx"].cuda())
    with torch.no_grad(), fused.precision(precision), native(**native_kv), _lib.timed_calls() as t:
        got = fused.sa_forward(sa, xyz, feats, new_xyz=new_xyz, idxs=[idx])[1]
    names = [r[0] for r in t.results() if r[0].startswith("g4d_mlp_")]
    assert names == [expect_family], names
    want = T.want(case, precision)[0].view(inp["B"], inp["P"], -1)
    if rep > 1:
        want = want.expand(rep, *want.shape[1:])
    same(got, want, f"{case['id']} ({precision})")


@pytest.mark.parametrize("case", T.SA_CASES, ids=lambda c: c["id"])
def test_sa_group_bf16_is_exact(case):
    """csrc/sa_group_bf16.hip, every instantiation, through fused.sa_forward: the launch goes to the bf16 chain entry point, whose persistent
    kernel takes it (switched on, row threshold 0, an instantiated (T1, S, C)); the small sizes run the register-chain kernel as well."""
    sh = case["shape"]
    assert (sh["C"] % 32 == 0 and (case["widths"][1] // 16, sh["S"], sh["C"]) in
            {(1, 16, 0), (2, 32, 0), (2, 16, 96), (4, 32, 96), (4, 32, 192), (8, 64, 192)}), "not an instantiation of sa_group_bf16_try"
    run_sa(case, "bf16", "g4d_mlp_chain_bf16", sa_group_bf16_persistent=1, sa_group_bf16_min_rows=0)
    if case.get("rep", 1) == 1:
        run_sa(case, "bf16", "g4d_mlp_chain_bf16", sa_group_bf16_persistent=0)


def fp_inputs(inp):
    B, n, m = inp["B"], inp["n"], inp["m"]
    unknown = torch.from_numpy(syn.unit_cloud(B, n, seed=n)).cuda()
    known = unknown[:, :m].contiguous()              # only its shape is used: the search result is given
    return unknown, known, dev(inp["skip"]), dev(inp["known"]), (dev(inp["dist2"]), inp["nn_idx"].cuda().contiguous())


def fp_module(case, stack, nfp):
    w = case["widths"]
    fp = PM.PointnetFPModule(mlp=list(w[:nfp + 1]), bn=False)
    load_blocks(list(fp.mlp.children()), stack[:nfp])
    return fp.cuda().eval()


@pytest.mark.parametrize("order", ["plain", "cells"])
@pytest.mark.parametrize("case", T.FP_HEAD_CASES, ids=lambda c: c["id"])
def test_fp_head_bf16_is_exact(case, order):
    """csrc/fp_head_bf16.hip through fused.fp_forward(..., head=): the FP output (the tapped layer) and the logits, rows in place and in the cell
    order of the unknown cloud's ball grid; the register-chain kernel on the same launch as well."""
    inp, stack = T.build(case)
    fp = fp_module(case, stack, 2)
    head = torch.nn.Sequential(pt_utils.Conv1d(64, 32, bn=False), torch.nn.Dropout(), pt_utils.Conv1d(32, 7, activation=None))
    load_blocks(list(head.children()), stack[2:])
    head = head.cuda().eval()
    unknown, known, _, kf, nn = fp_inputs(inp)
    grid = fused.build_ball_grid(unknown, 0.1) if order == "cells" else None
    want, want_tap = T.want(case, "bf16")
    for on in (1, 0):
        with torch.no_grad(), fused.precision("bf16"), native(fp_head_bf16_persistent=on, fp_head_bf16_min_rows=0), _lib.timed_calls() as t:
            feats, logits = fused.fp_forward(fp, unknown, known, None, kf, head=head, unknown_grid=grid, nn=nn)
        names = [r[0] for r in t.results() if r[0].startswith("g4d_mlp_")]
        assert names == ["g4d_mlp_chain_cells_bf16" if grid is not None else "g4d_mlp_chain_bf16"], names
        same(feats.view(-1, 64), want_tap, f"{case['id']} FP output (persistent kernel {on}, {order})")
        same(logits.view(-1, 7), want, f"{case['id']} logits (persistent kernel {on}, {order})")


@pytest.mark.parametrize("case", T.GEMM_CASES, ids=lambda c: c["id"])
def test_gemm_bf16_is_exact(case, tune):
    """csrc/gemm_bf16.hip: the wide FP level as an interpolation pre-pass and two tiled bf16 GEMMs."""
    inp, stack = T.build(case)
    fp = fp_module(case, stack, 2)
    unknown, known, skip, kf, nn = fp_inputs(inp)
    tune(fp_gemm_bf16=True)
    tune(fp_gemm_bf16_min_rows=0)
    with torch.no_grad(), fused.precision("bf16"), _lib.timed_calls() as t:
        got = fused.fp_forward(fp, unknown, known, skip, kf, nn=nn)
    names = [r[0] for r in t.results()]
    assert names.count("g4d_gemm_frag_bf16") == 2 and not any(n.startswith("g4d_mlp_") for n in names), names
    same(got.view(inp["rows"], -1), T.want(case, "bf16")[0], case["id"])


MODULE_RUNS = [(c, p) for c in T.MODULE_CASES for p in c["precisions"]]


@pytest.mark.parametrize("case,precision", MODULE_RUNS, ids=[f"{c['id']}-{p}" for c, p in MODULE_RUNS])
def test_public_routes_onto_widths_without_a_bf16_instantiation(case, precision):
    """An SA module with mlp = [C, 32, 64], an FP module and an FC stack with a single 256-wide layer in "bf16" / "bf16x3": the bf16 chain entry
    point has no instantiation for these widths (it used to launch one on null pointers); "bf16" takes the LDS stack kernel and "bf16x3" the
    fp32 chain kernel, both exact here."""
    fam = "g4d_mlp_stack_bf16" if precision == "bf16" else "g4d_mlp_chain_f32"
    if case["kind"] == "group":
        return run_sa(case, precision, fam)
    inp, stack = T.build(case, precision)
    want = T.want(case, precision)[0]
    with torch.no_grad(), fused.precision(precision), _lib.timed_calls() as t:
        if case["kind"] == "interp":
            fp = fp_module(case, stack, 1)
            unknown, known, skip, kf, nn = fp_inputs(inp)
            got = fused.fp_forward(fp, unknown, known, skip, kf, nn=nn)
        else:
            fc = torch.nn.Sequential(pt_utils.Conv1d(case["widths"][0], case["widths"][1], bn=False))
            load_blocks(list(fc.children()), stack)
            got = fused.conv_stack_forward(fc.cuda().eval(), dev(inp["X"]).view(1, inp["rows"], -1))
    names = [r[0] for r in t.results() if r[0].startswith("g4d_mlp_")]
    assert names == [fam], names
    same(got.view(inp["rows"], -1), want, f"{case['id']} ({precision})")
