"""The positional encoder's forward (csrc/pos_encode.hip, g4d_pos_encode_f32) alone, against the float64 twin of tests/refine_grad_twin.py within
the bound derived there (pe_forward_bound: nothing in it is a measured number), at sizes where a wave's chunk of 64 grouped rows straddles
two frames and the launch ends in a partial chunk -- every other test of the suite has Vg * nsample % 64 == 0.  tests/test_pos_encode_cpu.py
ties the same twin and bound to the oracle.  Each comparison prints its worst err / bound and asserts err <= bound for every element."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import refine_grad_twin as TW
from garment4d_amd import _lib
from garment4d_amd import refine as R

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.678)
VARIANTS = {"plain0": (0, False), "plain1": (1, False), "plain2": (2, False), "plain3": (3, False), "plain4": (4, False), "plain5": (5, False),
            "table": (0, True)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def seed_of(S, variant, base=0):
    return base + 10 * S + sorted(VARIANTS).index(variant)


def mlp_of(c):
    """Sequential(Linear(3 + E, 32), ReLU, Linear(32, 32)) carrying the case's weights (with a raw table: the coordinate columns, bias unused)."""
    E = c["E"]
    mlp = torch.nn.Sequential(torch.nn.Linear(3 + E, 32), torch.nn.ReLU(), torch.nn.Linear(32, 32))
    with torch.no_grad():
        mlp[0].weight.copy_(torch.from_numpy(c["W1"]))
        mlp[0].bias.copy_(torch.from_numpy(c["b1"]) if c["b1"] is not None else torch.zeros(32))
        mlp[2].weight.copy_(torch.from_numpy(c["W2"]))
        mlp[2].bias.copy_(torch.from_numpy(c["b2"]))
    return mlp.cuda()


def run_pe(c, ldo=32, col0=0, kernel_only=True, mlp=None, feats=None, table=None):
    """One refine.positional_encoding call into the window [col0, col0 + 32) of rows `ldo` floats wide pre-filled with SENTINEL; asserts that
    the columns outside the window keep the sentinel's bits.  Returns the window (F,P,32) as numpy."""
    xyz, q, idx = dev(c["xyz"]), dev(c["new_xyz"]), dev(c["idx"])
    if feats is None:
        feats = dev(c["extra"]) if c["E"] else torch.empty((c["F"], c["N"], 0), device="cuda")
    if table is None and c["table"] is not None:
        table = dev(c["table"])
    out = torch.full((c["F"], c["P"], ldo), float(SENTINEL), device="cuda")
    with torch.no_grad():
        R.positional_encoding(mlp_of(c) if mlp is None else mlp, None, c["S"], xyz, q, feats, out, col0, idx=idx, table=table, _kernel_only=kernel_only)
    torch.cuda.synchronize()
    assert bool((out[..., :col0] == float(SENTINEL)).all()) and bool((out[..., col0 + 32:] == float(SENTINEL)).all()), "a column outside the window was written"
    return out[..., col0:col0 + 32].contiguous().cpu().numpy()


def hold(what, got, c, frames=None, table_err=None):
    """got (len(frames),P,32) within the derived bound of the float64 twin, element by element; returns the worst err / bound."""
    ref, bnd = TW.pe_twin(c, frames=frames, table_err=table_err)
    assert got.shape == ref.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bnd)                                           # a NaN in `got` counts as beyond
    worst = float(np.nanmax(err / bnd))
    print(f"[pe-forward] {what}: worst err / bound = {worst:.4f} (max |ref| = {np.abs(ref).max():.3e})")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {err.size} elements beyond the derived bound (worst ratio {worst:.3g}); first at {np.argwhere(bad)[0].tolist()}"
    assert (ref != np.asarray(c["b2"], np.float64)).mean() > 0.5, "degenerate case: the ReLU killed everything"
    return worst


def case_of(S, variant, F_=3, N=301, P=259, base=0, **kw):
    E, table = VARIANTS[variant]
    return TW.pe_case(seed_of(S, variant, base), F_, N, P, S, E, table, **kw)


# ---- the variant matrix -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variant_matrix_against_float64(S, variant):
    """F = 3, N = 301, P = 259: P * S is no multiple of 64 for S <= 32 (chunks straddle frames, the launch ends in a partial chunk; S = 64:
    whole chunks, three frames).  Written at column 5 of rows 77 floats wide."""
    P = 259
    assert (P * S) % 64 != 0 or S == 64
    c = case_of(S, variant, P=P)
    hold(f"matrix S={S} {variant}", run_pe(c, ldo=77, col0=5), c)


# ---- frame straddle, made visible ---------------------------------------------------------------------------------------------------------
def shift_frames(c):
    """Frames that differ grossly: frame f's source coordinates and extra columns / table shifted by 10 f."""
    for k in ("xyz", "extra", "table"):
        if c[k] is not None:
            c[k] = (c[k] + 10.0 * np.arange(c["F"], dtype=np.float32).reshape(-1, 1, 1)).astype(np.float32)
    return c


STRADDLE_P = {4: 67, 8: 35, 16: 19, 32: 9}


@pytest.mark.parametrize("S", [4, 8, 16, 32])
@pytest.mark.parametrize("variant", ["plain0", "plain3", "plain5", "table"])
def test_frame_boundary_inside_a_chunk(S, variant):
    """The frame boundary falls inside a 16-row tile (S = 4, 8) or between the tiles of one chunk (S = 16, 32); a row attributed to the
    neighbouring frame reads coordinates 10 away."""
    P = STRADDLE_P[S]
    rows = P * S
    if S <= 8:
        assert rows % 16 == {4: 12, 8: 8}[S]
    else:
        assert rows % 16 == 0 and rows % 64 == {16: 48, 32: 32}[S]
    assert rows >= 64
    c = shift_frames(case_of(S, variant, P=P, base=1000))
    hold(f"straddle S={S} P={P} {variant}", run_pe(c, ldo=40, col0=3), c)


@pytest.mark.parametrize("S", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("variant", ["plain3", "table"])
def test_smallest_legal_launch(S, variant):
    """P * S == 64 exactly, five frames: one whole chunk per frame."""
    P = 64 // S
    c = shift_frames(case_of(S, variant, F_=5, P=P, base=2000))
    assert c["P"] * c["S"] == 64
    hold(f"smallest S={S} P={P} {variant}", run_pe(c), c)


@pytest.mark.parametrize("P", [17, 31, 33])
@pytest.mark.parametrize("variant", ["plain3", "table"])
def test_nsample4_odd_frames(P, variant):
    """S = 4 with 68, 124, 132 rows per frame."""
    c = shift_frames(case_of(4, variant, P=P, base=3000 + P))
    assert c["P"] * 4 in (68, 124, 132)
    hold(f"S=4 P={P} {variant}", run_pe(c, ldo=35, col0=2), c)


# ---- exact placement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_exact_placement(S, variant):
    """Integer-valued operands whose every partial sum is an integer below 2^24 (TW.pe_exact_case): the kernel's output equals the float64
    result bit for bit.  A swapped channel of the fragment layout, a wrong k-step of layer 1 or a sample attributed to the neighbouring
    query cannot hide behind a tolerance."""
    E, table = VARIANTS[variant]
    P = 259
    assert (P * S) % 64 != 0 or S == 64
    c = TW.pe_exact_case(seed_of(S, variant, 4000), 3, 301, P, S, E, table)
    want = TW.pe_exact_expected(c)
    got = run_pe(c, ldo=77, col0=5)
    diff = got.astype(np.float64) != want
    assert not diff.any(), f"S={S} {variant}: {int(diff.sum())} of {diff.size} elements differ; first at {np.argwhere(diff)[0].tolist()}"


# ---- padding and ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain3", "table"])
def test_all_samples_one_source_point(variant):
    """Every sample of a query is the same source point (an empty ball: ball_query leaves index 0 everywhere; and a random point per query):
    the result is the single-row value -- within the bound of the twin evaluated on ONE row, and the same bits for every nsample."""
    first = {}
    for fill in ("zero", "random"):
        for S in (4, 8, 16, 32, 64):
            c = case_of(32, variant, base=5000)                   # the same tensors for every S
            one = np.zeros((c["F"], c["P"], 1), np.int32) if fill == "zero" else c["idx"][..., :1]
            c["S"], c["idx"] = S, np.ascontiguousarray(np.broadcast_to(one, (c["F"], c["P"], S)))
            got = run_pe(c, ldo=40, col0=4)
            single = dict(c, S=1, idx=one)
            hold(f"one source point ({fill}) S={S} {variant}", got, single)
            assert np.array_equal(first.setdefault(fill, got), got), f"S={S}: copies of one row must give the row's own value, whatever nsample"


@pytest.mark.parametrize("S", [8, 32])
@pytest.mark.parametrize("variant", ["plain3", "table"])
def test_padding_heavy_rows(S, variant):
    """Queries with 1 .. 3 distinct hits, the rest copies of the first."""
    c = case_of(S, variant, base=6000, hits=3)
    assert (c["idx"][..., 3:] == c["idx"][..., :1]).all()
    hold(f"padding-heavy S={S} {variant}", run_pe(c), c)


# ---- many chunks per wave -----------------------------------------------------------------------------------------------------------------
def test_many_chunks_per_wave():
    """21 008 chunks of 64 rows, more than twice the 8192 waves of the capped grid (2048 workgroups of 4 waves): the persistent loop's second
    and third trips, both row buffers of the pipelined form, a clamped chunk past a wave's last one.  Ragged: 4099 * 8 % 64 == 24 rows of
    every frame's last chunk belong to it, and 41 frames leave the launch a partial last chunk of 24 rows."""
    F_, N, P, S = 41, 6890, 4099, 8
    rows = F_ * P * S
    assert (P * S) % 64 == 24 and rows % 64 == 24 and (rows + 63) // 64 == 21008 > 2 * 8192
    c = TW.pe_case(71, F_, N, P, S, 3, False)
    hold("many chunks F=41 P=4099 S=8 plain3", run_pe(c, ldo=36, col0=1), c)


def test_full_cfg4_launch_on_sampled_frames():
    """One body encoder's launch at cfg4: 240 frames x 4096 queries x 8 samples over 6890 body vertices with normals, written at column 3 of
    196-float rows; the float64 side checks the first frame, the last and two in between."""
    F_ = 240
    c = TW.pe_case(5, F_, 6890, 4096, 8, 3, False)
    xyz, q, idx, feats = dev(c["xyz"]), dev(c["new_xyz"]), dev(c["idx"]), dev(c["extra"])
    out = torch.full((F_, 4096, 196), float(SENTINEL), device="cuda")
    with torch.no_grad():
        R.positional_encoding(mlp_of(c), None, 8, xyz, q, feats, out, 3, idx=idx, _kernel_only=True)
    torch.cuda.synchronize()
    assert bool((out[..., :3] == float(SENTINEL)).all()) and bool((out[..., 35:] == float(SENTINEL)).all())
    frames = [0, 79, 160, 239]
    hold("cfg4 body encoder S=8, frames 0 / 79 / 160 / 239", out[frames][..., 3:35].contiguous().cpu().numpy(), c, frames=frames)


# ---- containment of a non-finite source point ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 32])
@pytest.mark.parametrize("variant", ["plain0", "plain3", "table"])
def test_nonfinite_source_point_is_contained(S, variant):
    """One source point's coordinates set to NaN, then to +inf: every query whose index row does not name that point keeps the clean run's
    bits.  What the queries that DO name it return is not pinned here: the kernel's fmaxf drops a NaN where the reference's max propagates
    it, by design (see the non-finite test of tests/test_large_launch_gpu.py)."""
    c = case_of(S, variant, base=7000)
    clean = run_pe(c)
    f, j = 1, int(c["idx"][1, 100, 0])
    names = (c["idx"] == j).any(-1)
    names[np.arange(c["F"]) != f] = False                         # (F,P): the queries of frame f that name point j
    assert 0 < names.sum() < c["P"]
    for bad in (np.nan, np.inf):
        d = dict(c, xyz=c["xyz"].copy())
        d["xyz"][f, j] = bad
        got = run_pe(d)
        same = got.view(np.uint32) == clean.view(np.uint32)
        assert same[~names].all(), f"{bad}: {int((~same[~names]).sum())} elements of queries that do not name the point changed"


# ---- the other builds of the loop ---------------------------------------------------------------------------------------------------------
BUILD_CASES = [(S, v) for S in (8, 32) for v in ("plain0", "plain3", "plain5", "table")]


def build_outputs():
    """The reduced matrix (ragged P = 259) under whatever build of the loop this process selected: (8,F,P,32)."""
    return np.stack([run_pe(case_of(S, v, base=8000), ldo=77, col0=5) for S, v in BUILD_CASES])


def child_main(path):
    np.save(path, build_outputs())


def test_the_four_builds_of_the_loop():
    """G4D_PE_PIPE x G4D_PE_L1_MFMA are read once per process: each combination runs in a fresh child process, one after the other; the
    first child that does not exit with 0 ends the test and no further one is started.  Every build is held to the float64 bound;
    csrc/pos_encode.hip states that the forms are bit-identical, so their bits are compared with the default build's too."""
    assert "G4D_PE_PIPE" not in os.environ and "G4D_PE_L1_MFMA" not in os.environ, "this process must run the default build"
    default = build_outputs()
    outs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for pipe in (1, 0):
            for l1m in (1, 0):
                path = os.path.join(tmp, f"pe_{pipe}{l1m}.npy")
                env = dict(os.environ, G4D_PE_PIPE=str(pipe), G4D_PE_L1_MFMA=str(l1m))
                code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_pos_encode_gpu as t; "
                        f"t.child_main({path!r})")
                r = subprocess.run([sys.executable, "-c", code], env=env, timeout=600, capture_output=True, text=True)
                assert r.returncode == 0, f"child PIPE={pipe} L1_MFMA={l1m} exited with {r.returncode}: {r.stderr[-2000:]}"
                outs[(pipe, l1m)] = np.load(path)
    for key, o in outs.items():
        for i, (S, v) in enumerate(BUILD_CASES):
            hold(f"build PIPE={key[0]} L1_MFMA={key[1]} S={S} {v}", o[i], case_of(S, v, base=8000))
    differing = {f"PIPE={k[0]} L1_MFMA={k[1]}": int((o.view(np.uint32) != default.view(np.uint32)).sum()) for k, o in outs.items()}
    print(f"[pe-forward] elements whose bits differ from the default build: {differing}")
    assert not any(differing.values()), differing


# ---- the generic route --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 32, 12])
def test_generic_route_against_float64(S, tune):
    """use_pe_kernel = False sends the kernel's own shapes to the fused stack with the pool in the launch (S = 8, 32: fused.stack_fits); an
    nsample the kernel does not take (12) goes there whatever the switch, through the un-pooled stack and the row-pool kernel."""
    from garment4d_amd import fused
    c = TW.pe_case(9000 + S, 3, 301, 259, S, 3, False)
    mlp = mlp_of(c)
    assert fused.stack_fits(R._pack_linear_mlp(mlp), 1, S, rows=3 * 259 * S) == (S != 12)
    if S != 12:
        tune(use_pe_kernel=False)
    hold(f"generic S={S} plain3", run_pe(c, ldo=77, col0=5, kernel_only=False, mlp=mlp), c)


def feature_case(seed, C, S, F_=3, N=301, P=259):
    """An encoder whose first Linear is C wide (3 coordinates + C - 3 features): the case, its module and features, the fp32 table of
    refine.feature_table and the twin's table error."""
    c = TW.pe_case(seed, F_, N, P, S, 0, False)
    rng = np.random.default_rng(seed + 1)
    feats = rng.standard_normal((F_, N, C - 3)).astype(np.float32)
    Wf = (rng.uniform(-1, 1, (32, C - 3)) / np.sqrt(C)).astype(np.float32)
    mlp = torch.nn.Sequential(torch.nn.Linear(C, 32), torch.nn.ReLU(), torch.nn.Linear(32, 32))
    with torch.no_grad():
        mlp[0].weight.copy_(torch.from_numpy(np.concatenate([c["W1"], Wf], 1)))
        mlp[0].bias.copy_(torch.from_numpy(c["b1"]))
        mlp[2].weight.copy_(torch.from_numpy(c["W2"]))
        mlp[2].bias.copy_(torch.from_numpy(c["b2"]))
    mlp = mlp.cuda()
    t64, terr = TW.table_forward(feats, Wf, c["b1"])
    c["table"], c["b1"] = t64, None                               # the twin: the exact table, its fp32 error carried in table_err
    return c, mlp, dev(feats), terr


@pytest.mark.parametrize("C", [67, 387])
@pytest.mark.parametrize("route", ["kernel", "stack", "stack12"])
def test_table_from_features_against_float64(C, route, tune):
    """The table built by refine.feature_table (its own contraction error added to layer 1's error term), consumed by the dedicated kernel,
    by the fused stack (use_pe_kernel = False) and by the un-pooled stack (nsample 12)."""
    S = 12 if route == "stack12" else 8
    c, mlp, feats, terr = feature_case(9500 + C + S, C, S)
    if route == "stack":
        tune(use_pe_kernel=False)
    with torch.no_grad():
        table = R.feature_table(mlp, feats)
    err_t = np.abs(table.cpu().numpy().astype(np.float64) - c["table"])
    assert (err_t <= terr).all(), "feature_table beyond its own bound"
    got = run_pe(c, ldo=77, col0=5, kernel_only=route == "kernel", mlp=mlp, feats=feats, table=table)
    hold(f"table from C={C} features, {route}", got, c, table_err=terr)


# ---- small meshes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,S", [(5, 8), (1, 32)])
@pytest.mark.parametrize("variant", ["plain3", "table67"])
def test_fewer_than_64_rows_per_frame(P, S, variant):
    """P * S < 64: a wave's chunk would span more than two frames and the kernel's launcher refuses the call; positional_encoding takes the
    generic stack and returns the twin's values."""
    assert P * S < 64
    with pytest.raises(_lib.G4DError):                            # the launcher's own limit, unchanged
        z = torch.zeros(8, device="cuda")
        _lib.call("g4d_pos_encode_f32", 3, 301, P, S, 0, *([z.data_ptr()] * 3), 0, *([z.data_ptr()] * 6), 32, 0, _lib.stream_ptr())
    if variant == "plain3":
        c = TW.pe_case(9900 + S, 3, 301, P, S, 3, False)
        hold(f"small mesh P={P} S={S} plain3", run_pe(c, ldo=40, col0=5, kernel_only=False), c)
    else:
        c, mlp, feats, terr = feature_case(9950 + S, 67, S, P=P)
        with torch.no_grad():
            table = R.feature_table(mlp, feats)
        hold(f"small mesh P={P} S={S} table", run_pe(c, ldo=40, col0=5, kernel_only=False, mlp=mlp, feats=feats, table=table), c, table_err=terr)
