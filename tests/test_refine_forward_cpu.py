"""tests/refine_forward_twin.py without a GPU.  (1) Each twin is tied to what exists: the GCN oracle on a mesh adjacency, the float64 torch
expression of test_temporal_attention_kernels.  (2) For every case of tests/test_refine_forward_gpu.py a plain fp32 numpy restatement of the
kernel's operation order stays inside the derived bound (a correct implementation passes) and the bound is below the case's signal (it is not
vacuous).  (3) Every case's precondition is asserted with tile_plan / attention_layout, so that no case can pass on the wrong path.  (4) The
argument refusals that come before any launch."""
import math

import numpy as np
import pytest
import torch

import refine_forward_twin as T
from garment4d_amd import _lib, synthetic as syn
from oracle import gcn_oracle

F32, F64 = np.float32, np.float64
TILES = (128, 64)


# ------------------------------------------------------------------------------------------------------------- fp32 restatements
def fma32(a, b, c):
    """fmaf in numpy: the product of two fp32 numbers is exact in float64; the sum is rounded to 53 bits and then to 24 (a double rounding
    fmaf does not have: the restatements need not be bit-exact)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def spmm_rows_f32(S, rowptr, colidx, vals, bias, relu):
    """spmm_rows_kernel's order: acc = fmaf(w, x, acc) in CSR order from 0, + bias (or + 0), fmaxf."""
    F_, vg, c = S.shape
    out = np.zeros((F_, vg, c), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(vg):
            acc = np.zeros((F_, c), F32)
            for e in range(int(rowptr[r]), int(rowptr[r + 1])):
                acc = fma32(vals[e], S[:, colidx[e], :], acc)
            y = acc + (bias if bias is not None else F32(0))
            out[:, r] = np.fmax(y, F32(0)) if relu else y
    return out


def contract_f32(h, W):
    """The assumed worst case of the MFMA chain: every product rounded, added to the accumulator one after another, every addition rounded."""
    acc = np.zeros(h.shape[:-1] + (W.shape[1],), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(W.shape[0]):
            acc = acc + h[..., k:k + 1] * W[k]
    return acc


def attention_f32(qkv, nclips, Tn, Vg, C):
    """attention.hip's order: per wave a chain over its 512 products, ((w0 + w1) + w2) + w3, four chains over the workgroups with the remainder
    on chain 0, (s0 + s1) + (s2 + s3), / (float)sqrt(T); max, expf(s - m) summed in order, one division; T fused steps per output."""
    ksteps, slices, wgs = T.attention_layout(Vg, C)
    D, L = Vg * C, T.K_STEPS * 16
    x = qkv.reshape(nclips, Tn, Vg, 3, C)
    q, k, v = (np.ascontiguousarray(x[:, :, :, i, :]).reshape(nclips, Tn, D) for i in range(3))
    pad = wgs * 4 * L - D
    qp = np.pad(q, ((0, 0), (0, 0), (0, pad))).reshape(nclips, Tn, wgs * 4, L)
    kp = np.pad(k, ((0, 0), (0, 0), (0, pad))).reshape(nclips, Tn, wgs * 4, L)
    acc = np.zeros((nclips, wgs * 4, Tn, Tn), F32)
    for j in range(L):
        acc = acc + qp[:, :, :, j].transpose(0, 2, 1)[..., :, None] * kp[:, :, :, j].transpose(0, 2, 1)[..., None, :]
    w = acc.reshape(nclips, wgs, 4, Tn, Tn)
    part = ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]
    s = [np.zeros((nclips, Tn, Tn), F32) for _ in range(4)]
    i = 0
    while i + 3 < wgs:
        for c in range(4):
            s[c] = s[c] + part[:, i + c]
        i += 4
    while i < wgs:
        s[0] = s[0] + part[:, i]
        i += 1
    sc = ((s[0] + s[1]) + (s[2] + s[3])) / F32(math.sqrt(float(Tn)))
    e = np.exp((sc - sc.max(-1, keepdims=True)).astype(F32)).astype(F32)
    z = np.zeros((nclips, Tn), F32)
    for j in range(Tn):
        z = z + e[..., j]
    att = (e / z[..., None]).astype(F32)
    out = np.zeros((nclips, Tn, D), F32)
    for u in range(Tn):
        out = fma32(att[:, :, u, None], v[:, None, u, :], out)
    return att, out.reshape(nclips * Tn, Vg, C)


def below_signal(want, bound):
    fin = np.isfinite(want)
    return float(bound[fin].max()) < float(np.abs(want[fin]).max())


# ---------------------------------------------------------------------------------------------------------------- 1. twins vs oracle
def test_gcn_twins_agree_with_the_oracle_on_a_mesh_adjacency():
    """graph_convolution (fp32 numpy / scipy, un-fused: up to 2 n roundings per row) against spmm_rows_f64 within twice its bound, and the next
    layer's support against agg_linear_f64 at the oracle's own 1e-5."""
    verts, faces = syn.quad_cylinder(9, 7)
    vg = verts.shape[0]
    adj = gcn_oracle.adjacency_from_faces(faces, vg).tocsr()
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, vg, 40)).astype(F32)
    W1 = (rng.standard_normal((40, 128)) * 0.2).astype(F32)
    b1 = rng.standard_normal(128).astype(F32)
    W2 = (rng.standard_normal((128, 16)) * 0.1).astype(F32)
    S = np.matmul(x, W1).astype(F32)
    want = gcn_oracle.graph_convolution(x, W1, b1, adj)
    h, bound = T.spmm_rows_f64(S, adj.indptr, adj.indices, adj.data.astype(F32), b1, 0)
    assert (np.abs(want - h) <= 2.0 * bound).all()
    hr, out, bound_h, bound_out = T.agg_linear_f64(S, adj.indptr, adj.indices, adj.data.astype(F32), b1, 1, W2)
    assert np.array_equal(hr, np.maximum(h, 0)) and np.array_equal(bound_h, bound)
    want2 = np.matmul(np.maximum(want, 0), W2)                       # layers.py:42 of the next layer
    assert np.abs(want2 - out).max() <= 1e-5 * max(1.0, np.abs(out).max())
    assert below_signal(out, bound_out)


@pytest.mark.parametrize("nclips,Tn,Vg,C", [(2, 30, 30, 16), (1, 3, 17, 16), (3, 32, 8, 48)])
def test_attention_twin_agrees_with_float64_torch(nclips, Tn, Vg, C):
    qkv = torch.randn(nclips * Tn, Vg, 3 * C, generator=torch.Generator().manual_seed(Tn)) * 0.3
    q, k, v = [z.reshape(nclips, Tn, Vg * C).double() for z in qkv.reshape(nclips, Tn, Vg, 3 * C).chunk(3, -1)]
    want_att = torch.softmax(q @ k.transpose(1, 2) / Tn ** 0.5, -1)
    want = (want_att @ v).reshape(nclips * Tn, Vg, C)
    att, out, _, _ = T.attention_f64(qkv.numpy(), nclips, Tn, Vg, C)
    np.testing.assert_allclose(att, want_att.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(out, want.numpy(), rtol=1e-12, atol=1e-13)


def test_tile_plan_on_a_mesh():
    """The 64 x 64 quad cylinder the kernel was built for: every tile fast, windows of 128 + 2 * 65 rows at most (gcn_fused.hip head)."""
    verts, faces = syn.quad_cylinder(64, 64)
    adj = gcn_oracle.adjacency_from_faces(faces, 4096).tocsr()
    plan = T.tile_plan(adj.indptr, adj.indices, 4096, 128)
    assert len(plan) == 32 and all(fast for *_, fast in plan) and max(hi - lo for lo, hi, _, _ in plan) <= 258


# ------------------------------------------------------------------------------------------- 2. restatements inside the bounds: GCN
@pytest.mark.parametrize("c", T.SPMM_C)
@pytest.mark.parametrize("vg", [41, 1])
def test_spmm_restatement_within_bound(c, vg):
    k = T.spmm_case(c, vg)
    lens = np.diff(k["rowptr"])
    if vg > 1:
        assert {0, 1, 40} <= set(lens.tolist()) and lens[-1] == 0
    for bias in (None, k["bias"]):
        for relu in (0, 1):
            want, bound = T.spmm_rows_f64(k["S"], k["rowptr"], k["colidx"], k["vals"], bias, relu)
            ok, ratio = T.held(spmm_rows_f32(k["S"], k["rowptr"], k["colidx"], k["vals"], bias, relu), want, bound)
            assert ok, ratio
            assert below_signal(want, bound)


@pytest.mark.parametrize("tile", TILES)
def test_gcn_case_list_is_the_same_for_both_tiles(tile):
    names = T.gcn_case_names(tile)
    assert len(names) == len(set(names)) == 31
    assert [n for n in names if not n.startswith("vg_")] == [n for n in T.gcn_case_names(128) if not n.startswith("vg_")]
    assert [int(n[3:]) for n in names if n.startswith("vg_")] == [1, tile - 1, tile, tile + 1, 2 * tile + 1]


def _all_gcn():
    return [(tile, name) for tile in TILES for name in T.gcn_case_names(tile)]


@pytest.mark.parametrize("tile,name", _all_gcn())
def test_gcn_case_precondition_and_restatement(tile, name):
    c = T.gcn_case(name, tile)
    vg, frames, rowptr, colidx, vals = c["vg"], c["frames"], c["rowptr"], c["colidx"], c["vals"]
    assert vg <= 720 and frames <= 17 and c["S"].shape == (frames, vg, 128) and c["W"].shape == (128, c["cout"])
    assert rowptr[0] == 0 and rowptr[-1] == colidx.size == vals.size and colidx.min() >= 0 and colidx.max() < vg
    # ---- the precondition: which path every tile takes, and the limits the name promises
    plan = T.tile_plan(rowptr, colidx, vg, tile)
    exp = c["expect"]
    assert len(plan) == (vg + tile - 1) // tile
    for i, (lo, hi, ell, fast) in enumerate(plan):
        assert fast == (exp.get(i, "fast") == "fast"), (i, lo, hi, ell, fast)
        if fast:
            assert 0 <= lo < hi <= vg and hi - lo <= T.K_WIN[tile] and ell <= 8
    for i, n in exp.get("ell", {}).items():
        assert plan[i][2] == n
    for i, n in exp.get("win", {}).items():
        assert plan[i][1] - plan[i][0] == n
    if "total" in exp:
        assert frames * len(plan) == exp["total"] == int(name.split("_")[1])
    kind = name.split("_")[0]
    lens = np.diff(rowptr)
    if kind == "vg":
        assert vg == int(name[3:]) and frames == 2
    if name == "ell8":
        assert lens.max() == 8 and (lens[tile:2 * tile] == 8).sum() == 1
    if name == "ell9":
        assert lens.max() == 9 and set(range(1, 10)) <= set(lens[tile:2 * tile].tolist()) and lens[:tile].max() <= 7 and lens[2 * tile:].max() <= 7
    if kind == "win":
        assert T.K_WIN[tile] == {128: 288, 64: 224}[tile] and lens[tile:2 * tile].max() <= 7      # the window alone decides
    if name.startswith("empty_tiles"):
        assert plan[1][:2] == plan[3][:2] == (T.EMPTY_LO, 0) and len(plan) == 4 and vg % tile != 0
        assert (c["bias"] is None) == name.endswith("nobias") and c["relu"] == (c["bias"] is not None)
    if name == "empty_rows":
        assert all(lens[r] == 0 for r in c["empty"]) and plan[0][3] == 1 and plan[1][3] == 0
        assert {0, tile - 1, tile, vg - 1} <= set(c["empty"]) and set(range(tile + 8, tile + 16)) <= set(c["empty"])
    if kind == "cout":
        assert c["cout"] == int(name[5:])
    if kind == "epi":
        assert (c["bias"] is not None, c["relu"], c["tap"]) == (name[5] == "1", int(name[7]), name[9] == "1")
    if kind == "nonfinite":
        assert np.isinf(c["S"][0]).any() and np.isnan(c["S"][0]).any() and np.isfinite(c["S"][1]).all()
        # the fast tile's +inf row is row 0 of its window, NaN sits in the window's last row; rows shorter than the tile's longest exist (they are padded)
        assert plan[0][0] == c["bad"]["inf"][0] == 0 and c["window_end"] == plan[0][1] - 1 and np.isnan(c["S"][0, c["window_end"]]).any()
        assert (lens[:tile] < plan[0][2]).sum() > tile // 2
        for i in (0, 1):
            lo, hi = plan[i][:2]
            rows = range(i * tile, min((i + 1) * tile, vg))
            for r_bad in (c["bad"]["inf"][i], c["bad"]["nan"][i]):
                assert lo <= r_bad < hi and not np.isfinite(c["S"][0, r_bad]).all()
                refs = [r for r in rows if r_bad in colidx[rowptr[r]:rowptr[r + 1]]]
                assert 0 < len(refs) < len(rows) // 2
    if name == "ell9":   # a GENERAL matrix: weights of both signs and above 1, columns out of order and repeated inside a row
        assert (vals < 0).any() and (vals > 1).any()
        assert any((np.diff(colidx[rowptr[r]:rowptr[r + 1]]) < 0).any() for r in range(vg))
        assert any(len(set(colidx[rowptr[r]:rowptr[r + 1]].tolist())) < lens[r] for r in range(vg))
    # ---- a plain fp32 restatement stays inside the bounds, and the bounds are below the signal
    h64, out64, bound_h, bound_out = T.agg_linear_f64(c["S"], rowptr, colidx, vals, c["bias"], c["relu"], c["W"])
    h32 = spmm_rows_f32(c["S"], rowptr, colidx, vals, c["bias"], c["relu"])
    ok, ratio = T.held(h32, h64, bound_h)
    assert ok, f"tap: worst err/bound {ratio}"
    ok, ratio = T.held(contract_f32(h32, c["W"]), out64, bound_out)
    assert ok, f"out: worst err/bound {ratio}"
    assert below_signal(h64, bound_h) and below_signal(out64, bound_out)
    if name.startswith("empty_tiles"):
        want = np.zeros(128) if c["bias"] is None else np.maximum(c["bias"].astype(F64), 0)
        for r in list(range(tile, 2 * tile)) + list(range(3 * tile, vg)):
            assert np.array_equal(h64[:, r], np.broadcast_to(want, (frames, 128)))
    if kind == "nonfinite":
        bad_rows = ~np.isfinite(h64[0]).all(-1)
        assert 0 < bad_rows[:tile].sum() < tile // 2 and 0 < bad_rows[tile:2 * tile].sum() < tile // 2 and np.isfinite(h64[1]).all()
        assert np.array_equal(~np.isfinite(out64[0]).all(-1), bad_rows)
        for b in (0, tile):
            assert h64[0, b + 30, 0] == np.inf and h64[0, b + 30, 1] != np.inf
            assert h64[0, b + 32, 0] == (0.0 if c["relu"] else -np.inf)
            assert h64[0, b + 34, 6] == 0.0 if c["relu"] else np.isnan(h64[0, b + 34, 6])


# -------------------------------------------------------------------------------------- 2./3. attention: layout, restatement, signal
def test_attention_case_list():
    names = T.attention_case_names()
    assert len(names) == len(set(names)) == 35


@pytest.mark.parametrize("name", T.attention_case_names())
def test_attention_case_precondition_and_restatement(name):
    c = T.attention_case(name)
    nclips, Tn, Vg, C = c["nclips"], c["T"], c["Vg"], c["C"]
    assert Vg * C <= 72000 and 1 <= Tn <= 32 and C % 16 == 0 and c["ldo"] >= c["col0"] + C
    ksteps, slices, wgs = T.attention_layout(Vg, C)
    assert int(_lib.lib().g4d_temporal_attention_scratch_floats(nclips, Vg, C)) == nclips * slices * 1024
    got = dict(ksteps=ksteps, slices=slices, wgs=wgs)
    for key, n in c["expect"].items():
        assert got[key] == n, (key, got)
    kind = name.split("_")[0]
    if kind in ("ksteps", "slices", "wgs", "T", "C"):
        assert int(name.split("_")[1]) == {"ksteps": ksteps, "slices": slices, "wgs": wgs, "T": Tn, "C": C}[kind]
    if name == "ksteps_33":
        assert slices == 2 and ksteps - T.K_STEPS == 1                # a tail slice of ONE k-step
    if name == "slices_5":
        assert wgs == 2 and wgs * 4 - slices == 3                     # three inactive waves in the last workgroup
    att64, out64, bound_att, bound_out = T.attention_f64(c["qkv"], nclips, Tn, Vg, C)
    s = (np.einsum("ctd,cud->ctu", *[c["qkv"].astype(F64).reshape(nclips, Tn, Vg, 3, C)[:, :, :, i].reshape(nclips, Tn, -1) for i in (0, 1)])
         / math.sqrt(Tn))
    if c["kind"] == "peaked":
        d = np.diagonal(s, axis1=1, axis2=2)
        assert 29.0 <= d.min() and d.max() <= 81.0 and np.abs(d[:, [0, -1]] - [30.0, 80.0]).max() < 0.01
        assert (att64.argmax(-1) == np.arange(Tn)).all() and (s.max(-1) - s.min(-1)).max() > 25
    elif c["kind"] == "uniform":
        assert np.array_equal(s, np.zeros_like(s)) and np.array_equal(att64, np.full_like(att64, 1.0 / Tn))
    elif Tn > 1:
        assert 0.5 < s.std() < 8.0 and att64.max() > 1.5 / Tn        # far from uniform, yet ds stays small
    if name == "clips":
        assert not np.array_equal(c["qkv"][:Tn], c["qkv"][Tn:2 * Tn])
    att32, out32 = attention_f32(c["qkv"], nclips, Tn, Vg, C)
    ok, ratio = T.held(att32, att64, bound_att)
    assert ok, f"att: worst err/bound {ratio}"
    ok, ratio = T.held(out32, out64, bound_out)
    assert ok, f"out: worst err/bound {ratio}"
    assert np.abs(att32.astype(F64).sum(-1) - 1.0).max() <= T.row_sum_tolerance(Tn)
    assert below_signal(att64, bound_att) and below_signal(out64, bound_out)
    assert (bound_att <= 0.1 * att64 + 1e-30).all()                   # tight everywhere: at most a tenth of each weight


# ------------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_before_any_launch():
    """Each returns the invalid-argument status with the existing message; none reaches a launch (no GPU here)."""
    L = _lib.lib()
    EINVAL = 10001
    gcn = lambda c, cout: (1, 8, c, 1, 1, 1, 1, 1, 1, 0, 1, cout, 1, 0)
    bad = [
        ("g4d_gcn_agg_linear_f32", gcn(128, 17), "Cout must be 128 or <= 16 (got 17)"),
        ("g4d_gcn_agg_linear_f32", gcn(128, 0), "Cout must be 128 or <= 16 (got 0)"),
        ("g4d_gcn_agg_linear_f32", gcn(64, 128), "support width must be 128 (got 64)"),
        ("g4d_gcn_agg_linear_meta_f32", gcn(128, 17)[:-1] + (1, 0), "Cout must be 128 or <= 16 (got 17)"),
        ("g4d_temporal_attention_f32", (1, 0, 8, 16, 1, 1, 1, 1, 16, 0, 0), "need 1 <= T <= 32"),
        ("g4d_temporal_attention_f32", (1, 4, 8, 16, 1, 1, 1, 1, 15, 0, 0), "bad arguments"),
        ("g4d_temporal_attention_f32", (1, 4, 8, 16, 1, 1, 1, 1, 19, 4, 0), "bad arguments"),
        ("g4d_temporal_attention_f32", (1, 4, 8, 16, 1, 1, 1, 1, 32, -1, 0), "bad arguments"),
    ]
    for name, args, needle in bad:
        rc = getattr(L, name)(*args)
        assert rc == EINVAL, (name, args, rc)
        msg = L.g4d_last_error().decode()
        assert needle in msg and msg.startswith(("g4d_gcn_agg_linear_f32", "g4d_temporal_attention_f32")), (name, msg)
