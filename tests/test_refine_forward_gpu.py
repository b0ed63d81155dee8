"""The forward kernels of the refinement head's inference path at their tile edges: g4d_spmm_rows_f32 (csrc/pointnet2_ops.hip),
g4d_gcn_agg_linear_f32 / g4d_gcn_agg_linear_meta_f32 / g4d_gcn_tile_meta_build in BOTH compiled tile sizes (csrc/gcn_fused.hip; the 64-row build
is selected by G4D_GCN_TILE=64, read once per process: one child process runs the whole case list) and g4d_temporal_attention_f32
(csrc/attention.hip) with its attention matrix, against the float64 references and derived bounds of tests/refine_forward_twin.py.
tests/test_refine_forward_cpu.py asserts every case's precondition (which tile is fast or slow, the window and row-length limits, the workgroup
counts) and that the bounds hold for a plain restatement and are not vacuous.  Every bounded test prints its worst err / bound ratio.

Equalities between routes (metadata or none, tap against the SpMM) are np.array_equal with NaN == NaN: the same values everywhere, a zero's sign
apart (a padded fmaf(0, 0, -0.0) gives +0.0)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import refine_forward_twin as T
from garment4d_amd import _lib, fused
from garment4d_amd import gcn as G
from garment4d_amd import synthetic as syn
from oracle import gcn_oracle

pytestmark = pytest.mark.gpu
F64 = np.float64
SENTINEL = -12345.5
TESTS = os.path.dirname(os.path.abspath(__file__))


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def sentinel(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.float32, device="cuda")


def csr_dev(c):
    return dev(c["rowptr"]), dev(c["colidx"]), dev(c["vals"])


# ============================================================================================================================== SpMM
@pytest.mark.parametrize("vg", [41, 1])
@pytest.mark.parametrize("c", T.SPMM_C)
def test_spmm_rows_vs_float64(c, vg):
    """g4d_spmm_rows_f32 at widths on both sides of the float4 path (c % 4 != 0: scalar), rows of 0, 1 and 40 entries, vg = 1, 3 frames,
    bias x relu: within gamma(n + 1) (sum |w x| + |b|) of float64, one guard row intact.
    Measured on MI355X: worst err / bound 0.87 (c = 128, vg = 41), 0.03 .. 0.40 at vg = 1: short rows leave the few roundings little room to cancel."""
    k = T.spmm_case(c, vg)
    S, (rowptr, colidx, vals), bias = dev(k["S"]), csr_dev(k), dev(k["bias"])
    rows = 3 * vg
    worst = 0.0
    for b in (None, bias):
        for relu in (0, 1):
            out = sentinel(rows + 1, c)
            _lib.call("g4d_spmm_rows_f32", 3, vg, c, S.data_ptr(), rowptr.data_ptr(), colidx.data_ptr(), vals.data_ptr(), 0 if b is None else b.data_ptr(),
                      relu, out.data_ptr(), _lib.stream_ptr())
            out = host(out)
            assert (out[rows:] == SENTINEL).all(), "the row behind the last one was written"
            want, bound = T.spmm_rows_f64(k["S"], k["rowptr"], k["colidx"], k["vals"], None if b is None else k["bias"], relu)
            ok, ratio = T.held(out[:rows].reshape(3, vg, c), want, bound)
            worst = max(worst, ratio)
            assert ok, f"bias {b is not None} relu {relu}: worst err/bound {ratio}"
    print(f"spmm c={c} vg={vg}: worst err/bound {worst:.4f}")


# ==================================================================================================================== fused GCN launch
def library_tile():
    """The tile size this PROCESS's library uses (G4D_GCN_TILE is read once): from the metadata size of a one-vertex mesh."""
    ints = int(_lib.lib().g4d_gcn_tile_meta_bytes(1)) // 4
    return {T.meta_ints(128): 128, T.meta_ints(64): 64}[ints]


def run_gcn_case(c):
    """Every launch of one case -> dict of host arrays: spmm (the SpMM's output), tap_nometa / out_nometa (g4d_gcn_agg_linear_f32), tap_meta /
    out_meta (g4d_gcn_agg_linear_meta_f32), hdr (tiles, 4) the metadata headers, guards (all guard stripes intact).  tap and out carry one
    sentinel row behind the last one, the metadata 8 sentinel ints."""
    frames, vg, cout, tile = c["frames"], c["vg"], c["cout"], c["tile"]
    rows = frames * vg
    S, (rowptr, colidx, vals) = dev(c["S"]), csr_dev(c)
    bias = None if c["bias"] is None else dev(c["bias"])
    bp = 0 if bias is None else bias.data_ptr()
    L = fused.PackedLayer(dev(c["W"]).t().contiguous(), torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda"), relu=False)
    csr = (rowptr.data_ptr(), colidx.data_ptr(), vals.data_ptr())
    st = _lib.stream_ptr()
    spmm = sentinel(rows + 1, 128)
    _lib.call("g4d_spmm_rows_f32", frames, vg, 128, S.data_ptr(), *csr, bp, c["relu"], spmm.data_ptr(), st)
    tiles = (vg + tile - 1) // tile
    ints = int(_lib.lib().g4d_gcn_tile_meta_bytes(vg)) // 4
    assert ints == tiles * T.meta_ints(tile), f"the library does not run {tile}-row tiles in this process"
    meta = torch.full((ints + 8,), -7, dtype=torch.int32, device="cuda")
    _lib.call("g4d_gcn_tile_meta_build", vg, *csr, meta.data_ptr(), st)
    res = dict(spmm=host(spmm)[:rows])
    guards = bool((spmm[rows:] == SENTINEL).all()) and bool((meta[ints:] == -7).all())
    for tag in ("nometa", "meta"):
        tap = sentinel(rows + 1, 128) if c["tap"] else None
        out = sentinel(rows + 1, cout)
        args = (frames, vg, 128, S.data_ptr(), *csr, bp, c["relu"], 0 if tap is None else tap.data_ptr(), L.Wf.data_ptr(), cout, out.data_ptr())
        if tag == "meta":
            _lib.call("g4d_gcn_agg_linear_meta_f32", *args, meta.data_ptr(), st)
        else:
            _lib.call("g4d_gcn_agg_linear_f32", *args, st)
        guards = guards and bool((out[rows:] == SENTINEL).all()) and (tap is None or bool((tap[rows:] == SENTINEL).all()))
        res["out_" + tag] = host(out)[:rows]
        if tap is not None:
            res["tap_" + tag] = host(tap)[:rows]
    res["hdr"] = host(meta[:ints]).reshape(tiles, T.meta_ints(tile))[:, :4]
    res["guards"] = np.array(guards)
    return res


def check_gcn_case(c, res):
    """-> (worst tap ratio, worst out ratio)."""
    name, tile, frames, vg, cout = c["name"], c["tile"], c["frames"], c["vg"], c["cout"]
    assert bool(res["guards"]), f"{name}: a guard stripe behind tap / out / the metadata was written"
    plan = np.array(T.tile_plan(c["rowptr"], c["colidx"], vg, tile), dtype=np.int64)
    assert np.array_equal(res["hdr"], plan), f"{name}: metadata headers\n{res['hdr']}\nplan\n{plan}"
    assert same(res["out_nometa"], res["out_meta"]), f"{name}: out differs between the metadata and the no-metadata route"
    h64, out64, bound_h, bound_out = T.gcn_reference(name, tile)
    r_tap = 0.0
    if c["tap"]:
        assert same(res["tap_nometa"], res["tap_meta"]), f"{name}: tap differs between the metadata and the no-metadata route"
        assert same(res["tap_meta"], res["spmm"]), f"{name}: tap is not the SpMM's output"
        ok, r_tap = T.held(res["tap_meta"].reshape(frames, vg, 128), h64, bound_h)
        assert ok, f"{name}: tap worst err/bound {r_tap}"
    else:
        assert "tap_meta" not in res
    ok, r_spmm = T.held(res["spmm"].reshape(frames, vg, 128), h64, bound_h)
    assert ok, f"{name}: spmm worst err/bound {r_spmm}"
    ok, r_out = T.held(res["out_meta"].reshape(frames, vg, cout), out64, bound_out)
    assert ok, f"{name}: out worst err/bound {r_out}"
    return max(r_tap, r_spmm), r_out


@pytest.mark.parametrize("name", T.gcn_case_names(128))
def test_gcn_agg_linear_tile128(name):
    """The default 128-row build (kWin = 288), one case of refine_forward_twin.gcn_case per test: the no-metadata and the metadata call give the same
    tap and out, tap is the SpMM's output, both are within bound_h / bound_out of float64 with the reference's non-finite pattern, the metadata
    headers equal tile_plan (so the intended path ran), the guard rows are intact.
    Measured on MI355X over the 31 cases: worst err / bound 0.92 (tap, tiles_9; 0.15 at vg_1) and 0.040 (out, empty_tiles_nobias; 0.012 .. 0.040): out
    sits low because gamma(129) charges 129 worst-case roundings to a 128-term sum whose real roundings largely cancel (and the MFMA may round less often
    than assumed)."""
    assert library_tile() == 128, "this test needs the default tile: run the suite without G4D_GCN_TILE"
    c = T.gcn_case(name, 128)
    r_tap, r_out = check_gcn_case(c, run_gcn_case(c))
    print(f"gcn tile 128 {name}: worst err/bound tap {r_tap:.4f} out {r_out:.4f}")


def child_main(path):
    """In the G4D_GCN_TILE=64 child: run every tile-64 case, save the raw results."""
    assert library_tile() == 64
    out = {}
    for name in T.gcn_case_names(64):
        for key, a in run_gcn_case(T.gcn_case(name, 64)).items():
            out[f"{name}/{key}"] = a
    torch.cuda.synchronize()
    np.savez(path, **out)


def test_gcn_agg_linear_tile64_build(tmp_path):
    """gcn_fused_kernel<8, 64>, <1, 64> and gcn_meta_kernel<64> (kWin = 224), which only G4D_GCN_TILE=64 selects: ONE fresh child process runs the
    same case list with the limits moved (tile edges 63 / 64 / 65, windows of 224 / 225 rows) and writes tap, out and the metadata headers; this
    process holds them to the twin exactly as the 128-row cases are.
    Measured on MI355X over the 31 cases: worst err / bound 0.89 (tap) and 0.038 (out); the child takes about 3 s."""
    path = str(tmp_path / "tile64.npz")
    code = f"import sys; sys.path[:0] = [{os.path.dirname(TESTS)!r}, {TESTS!r}]; import test_refine_forward_gpu as G; G.child_main(sys.argv[1])"
    flags = ["-s"] if sys.flags.no_user_site else []                  # the child sees the packages this process sees
    run = subprocess.run([sys.executable, *flags, "-c", code, path], env=dict(os.environ, G4D_GCN_TILE="64"), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    data = np.load(path)
    worst = [0.0, 0.0]
    for name in T.gcn_case_names(64):
        res = {k.split("/", 1)[1]: data[k] for k in data.files if k.startswith(name + "/")}
        r = check_gcn_case(T.gcn_case(name, 64), res)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"gcn tile 64, {len(T.gcn_case_names(64))} cases: worst err/bound tap {worst[0]:.4f} out {worst[1]:.4f}")


def test_gcn_empty_tiles_are_the_activated_bias():
    """A tile without any entry (slow path, zero trip count): exactly act(bias) in every row, exactly 0 without a bias, in tap; out is that row times
    the next weight, the same in every such row."""
    for name in ("empty_tiles_bias", "empty_tiles_nobias"):
        c = T.gcn_case(name, 128)
        res = run_gcn_case(c)
        tap = res["tap_meta"].reshape(c["frames"], c["vg"], 128)
        out = res["out_meta"].reshape(c["frames"], c["vg"], c["cout"])
        want = np.zeros(128, np.float32) if c["bias"] is None else np.maximum(c["bias"], 0)
        rows = list(range(128, 256)) + list(range(384, c["vg"]))
        assert (tap[:, rows] == want).all()
        assert (out[:, rows] == out[0, 128]).all() and (c["bias"] is not None or (out[:, rows] == 0).all())


# ================================================================================================================= gcn_stack_forward
def _stack_refs(layers, x, adj, tune, **kw):
    with torch.no_grad():
        got = G.gcn_stack_forward(layers, x, adj, **kw)
        tune(gcn_fuse_stack=False)
        ref = G.gcn_stack_forward(layers, x, adj, **kw)
    h, want = host(x), []
    for i, m in enumerate(layers):
        h = gcn_oracle.graph_convolution(h, host(m.weight), None if m.bias is None else host(m.bias), adj)
        if i + 1 < len(layers):
            h = np.maximum(h, 0)
        want.append(h)
    return got, ref, want


def _stack_mesh(seed, widths):
    verts, faces = syn.quad_cylinder(13, 11)
    vg = verts.shape[0]
    adj = gcn_oracle.adjacency_from_faces(faces, vg)
    torch.manual_seed(seed)
    layers = [G.GraphConvolution(a, b).cuda() for a, b in zip(widths[:-1], widths[1:])]
    x = torch.randn(2, vg, widths[0], generator=torch.Generator().manual_seed(seed + 1)).cuda()
    return adj, layers, x


def test_gcn_stack_forward_2d_input_with_a_tapped_layer(tune):
    """A 2-D input (one frame, no batch axis) through the fused route with `keep` naming a tapped layer: every returned tensor is 2-D and equals frame 0
    of the 3-D call's, the kept activation is the layer-by-layer route's bit for bit, and both agree with the oracle."""
    adj, layers, x = _stack_mesh(21, (40, 128, 128, 3))
    with torch.no_grad():
        full = G.gcn_stack_forward(layers, x[:1].contiguous(), adj, keep=(1,))
    got, ref, want = _stack_refs(layers, x[0].contiguous(), adj, tune, keep=(1,))
    assert got[0] is None and got[1].shape == (x.shape[1], 128) and got[2].shape == (x.shape[1], 3)
    assert torch.equal(got[1], full[1][0]) and torch.equal(got[2], full[2][0])
    assert torch.equal(got[1], ref[1])
    torch.testing.assert_close(got[2], ref[2], rtol=1e-5, atol=1e-5)
    for i in (1, 2):
        assert np.abs(host(got[i]) - want[i]).max() <= 1e-5 * max(1.0, np.abs(want[i]).max())


def test_gcn_stack_forward_fused_then_plain_launch(tune):
    """128 -> 16 -> 128 behind the first layer: the aggregation of the 128-wide layer is fused with the 16-wide contraction (the NT = 1 mapping), the 16-wide
    layer then takes the plain SpMM on the support it was handed, the last layer contracts and aggregates on its own."""
    adj, layers, x = _stack_mesh(22, (40, 128, 16, 128))
    got, ref, want = _stack_refs(layers, x, adj, tune, keep=(0, 1))
    assert torch.equal(got[0], ref[0])                                  # the tapped activation: the SpMM's arithmetic
    for i in (1, 2):
        torch.testing.assert_close(got[i], ref[i], rtol=1e-5, atol=1e-5)
    for i in range(3):
        assert np.abs(host(got[i]) - want[i]).max() <= 1e-5 * max(1.0, np.abs(want[i]).max())


# ========================================================================================================================= attention
def run_attention(c, qkv=None):
    """-> (att (nclips, T, T), out (nclips * T, Vg, ldo) with the sentinel columns still in it); asserts the guard stripes behind att and out."""
    nclips, Tn, Vg, C, ldo, col0 = c["nclips"], c["T"], c["Vg"], c["C"], c["ldo"], c["col0"]
    qkv = dev(c["qkv"] if qkv is None else qkv)
    scratch = torch.empty(int(_lib.lib().g4d_temporal_attention_scratch_floats(nclips, Vg, C)), device="cuda")
    att = sentinel(1, nclips * Tn * Tn + 8)
    out = sentinel(nclips * Tn * Vg + 1, ldo)
    _lib.call("g4d_temporal_attention_f32", nclips, Tn, Vg, C, qkv.data_ptr(), scratch.data_ptr(), att.data_ptr(), out.data_ptr(), ldo, col0, _lib.stream_ptr())
    att, out = host(att)[0], host(out)
    assert (att[nclips * Tn * Tn:] == SENTINEL).all(), "att was written behind its end"
    assert (out[nclips * Tn * Vg:] == SENTINEL).all(), "the row behind the last output row was written"
    out = out[:nclips * Tn * Vg].reshape(nclips * Tn, Vg, ldo)
    assert (out[..., :col0] == SENTINEL).all() and (out[..., col0 + C:] == SENTINEL).all(), "columns outside [col0, col0 + C) were written"
    return att[:nclips * Tn * Tn].reshape(nclips, Tn, Tn), out


@pytest.mark.parametrize("name", T.attention_case_names())
def test_temporal_attention_vs_float64(name):
    """g4d_temporal_attention_f32 through its C entry, the attention matrix included: att within bound_att and out within bound_out of float64
    (refine_forward_twin.attention_f64), rows of att summing to 1, sentinel columns and guard rows intact.  T on both sides of the 16-row tile, 1 / 15 /
    32 / 33 k-steps, 4 and 5 slices, 1..8 workgroups, C 16..256, column offsets 0 / 3 / 4 with and without a padded stride, a peaked softmax
    (diagonal scores 30..80) and a uniform one.
    Measured on MI355X over the 35 cases: worst err / bound 0.024 (att, ksteps_1; 0.0002 .. 0.007 elsewhere) and 0.042 (out, uniform_9): the score
    bound charges every one of up to ~520 roundings its worst case, so the ratio falls as D grows; |row sum - 1| reaches 0.26 of its tolerance."""
    c = T.attention_case(name)
    nclips, Tn, Vg, C, col0 = c["nclips"], c["T"], c["Vg"], c["C"], c["col0"]
    att, out = run_attention(c)
    att64, out64, bound_att, bound_out = T.attention_f64(c["qkv"], nclips, Tn, Vg, C)
    ok_a, r_att = T.held(att, att64, bound_att)
    ok_o, r_out = T.held(out[..., col0:col0 + C], out64, bound_out)
    sums = np.abs(att.astype(F64).sum(-1) - 1.0).max()
    print(f"attention {name}: worst err/bound att {r_att:.4f} out {r_out:.4f}; |row sum - 1| {sums:.3e} of {T.row_sum_tolerance(Tn):.3e}")
    assert ok_a, f"att worst err/bound {r_att}"
    assert ok_o, f"out worst err/bound {r_out}"
    assert sums <= T.row_sum_tolerance(Tn)
    if c["kind"] == "uniform":                                        # expf(0) = 1, Z = T exactly: the one division
        assert (att == np.float32(1.0) / np.float32(Tn)).all()


def test_temporal_attention_clips_are_independent():
    """Three clips of different data; replacing clip 1's frames leaves the att and out of clips 0 and 2 bit-identical and changes clip 1's."""
    c = T.attention_case("clips")
    Tn = c["T"]
    att, out = run_attention(c)
    other = np.array(c["qkv"], copy=True)
    other[Tn:2 * Tn] = other[Tn:2 * Tn][::-1] * np.float32(-0.75)
    att2, out2 = run_attention(c, other)
    for clip in (0, 2):
        assert np.array_equal(att[clip], att2[clip]) and np.array_equal(out[clip * Tn:(clip + 1) * Tn], out2[clip * Tn:(clip + 1) * Tn])
    assert not np.array_equal(att[1], att2[1]) and not np.array_equal(out[Tn:2 * Tn], out2[Tn:2 * Tn])
    assert not np.array_equal(att[0], att[1]) and not np.array_equal(att[0], att[2])
