"""Backward of the GCN layer (csrc/gcn_grad.hip behind tuning.Tuning.gcn_autograd).

Kernel level: g4d_spmm_rows_grad_f32 (dS), g4d_col_sum_rows_f32 (db), g4d_gemm_tn_f32 (dW) and the dX contraction (g4d_linear_f32 with W as
the transposed weight), each alone on its actual fp32 inputs against a dense float64 computation written here (tests/gcn_grad_twin.py), every
element within  (k + 2) 2^-24 sum |term|  -- the first-order bound of a k-term fp32 sum in ANY order (k = terms of that element, sum |term|
from the same float64 computation; the form of tests/test_backward_gpu.py).  Nothing in these bounds is a measured number.

Against the reference's autograd (tests/golden/gcn_grad.npz, tied to the float64 twin by tests/test_gcn_grad_cpu.py): per tensor
max |hip - ref64| <= 3 e_ref with e_ref = max |ref32 - ref64|, the reference's own fp32 rounding error; tensors with fewer than 1024
elements are held to the derived per-element bound instead (a maximum over a handful of elements is a poor yardstick).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_grad_twin as TW
from garment4d_amd import _lib, fused, tuning
from garment4d_amd import gcn as G
from garment4d_amd import synthetic as syn

pytestmark = pytest.mark.gpu

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def autograd_on():
    return tuning.use(tuning.current().replace(gcn_autograd=True))


def fixture_adj():
    _, o = TW.load()
    m = sp.csr_matrix((o["adj_val"], (o["adj_row"], o["adj_col"])), shape=(64, 64))
    return G.sparse_mx_to_torch_sparse_tensor(m), TW.dense_adjacency(o)


def assert_within(got, ref, k, abs_sum, what):
    bound = TW.sum_bound(k, abs_sum)
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > bound
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max err / bound = {worst:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {err.size} elements beyond (k + 2) 2^-24 sum|term| (worst ratio {worst:.3f})"


# ---- raw launches ------------------------------------------------------------------------------------------------------------------------
def hip_gemm_tn(X, fin, dS):
    """X (rows, ldx) fp32 on the device, its first `fin` columns contracted with dS (rows, cout) along the rows."""
    rows, ldx = X.shape
    cout = dS.shape[1]
    ws = torch.empty(max(int(_lib.lib().g4d_gemm_tn_ws_bytes(rows, fin, cout)) // 4, 1), device="cuda")
    dW = torch.full((fin, cout), float("nan"), device="cuda")
    _lib.call("g4d_gemm_tn_f32", rows, fin, ldx, cout, X.data_ptr(), dS.data_ptr(), ws.data_ptr(), dW.data_ptr(), _lib.stream_ptr())
    return dW


def hip_col_sum(dY, Y):
    rows, c = dY.shape
    ws = torch.empty(max(int(_lib.lib().g4d_col_sum_rows_ws_bytes(rows, c)) // 4, 1), device="cuda")
    db = torch.full((c,), float("nan"), device="cuda")
    _lib.call("g4d_col_sum_rows_f32", rows, c, dY.data_ptr(), 0 if Y is None else Y.data_ptr(), ws.data_ptr(), db.data_ptr(), _lib.stream_ptr())
    return db


def hip_spmm_grad(dY, Y, adj):
    B, N, c = dY.shape
    rp, ci, va, n = G._to_csr_t(adj, dY.device)
    assert n == N
    dS = torch.full((B, N, c), float("nan"), device="cuda")
    _lib.call("g4d_spmm_rows_grad_f32", B, N, c, dY.data_ptr(), 0 if Y is None else Y.data_ptr(), rp.data_ptr(), ci.data_ptr(), va.data_ptr(),
              dS.data_ptr(), _lib.stream_ptr())
    return dS


def slice_rows(rows, fin, cout):
    return int(_lib.lib().g4d_gemm_tn_slice_rows(rows, fin, cout))


def row_counts(fin, cout):
    s = slice_rows(1, fin, cout)
    assert s == slice_rows(3 * s + 17, fin, cout), "small launches share one slice length"
    return [1, 63, 64, 65, s - 1, s, s + 1, 3 * s + 17]


# ---- the opt-in ---------------------------------------------------------------------------------------------------------------------------
def test_default_raises_and_the_switch_enables():
    adj, _ = fixture_adj()
    layer = G.GraphConvolution(12, 20).cuda()
    layers = [G.GraphConvolution(12, 128).cuda(), G.GraphConvolution(128, 3).cuda()]
    x = torch.randn(3, 64, 12, device="cuda", requires_grad=True)
    assert tuning.current().gcn_autograd is False
    with pytest.raises(NotImplementedError):
        layer(x, adj)
    with pytest.raises(NotImplementedError):
        G.gcn_stack_forward(layers, x, adj)
    with autograd_on():
        y = layer(x, adj)
        z = G.gcn_stack_forward(layers, x, adj)[-1]
    assert y.requires_grad and z.requires_grad
    (y.sum() + z.sum()).backward()
    assert x.grad is not None and layer.weight.grad is not None and layer.bias.grad is not None and layers[0].weight.grad is not None
    with pytest.raises(NotImplementedError):   # and off again outside the block
        layer(x, adj)


def test_forward_under_autograd_is_bit_identical_to_no_grad():
    adj, _ = fixture_adj()
    torch.manual_seed(3)
    layer, nb = G.GraphConvolution(12, 20).cuda(), G.GraphConvolution(12, 3, bias=False).cuda()
    x = torch.randn(3, 64, 12, device="cuda")
    stack = [G.GraphConvolution(a, b).cuda() for a, b in zip(TW.WIDTHS[:-1], TW.WIDTHS[1:])]
    xs = torch.randn(2, 64, 323, device="cuda")
    xp = torch.zeros(2, 64, 324, device="cuda")
    xp[..., :323] = xs
    with torch.no_grad():
        want = [layer(x, adj), layer(x[0], adj), layer(x, adj, ismlp=True), layer(x, adj, relu=True), layer(x, adj, ismlp=True, relu=True), nb(x, adj)]
        want_stack = G.gcn_stack_forward(stack, xs, adj, keep=(0, 1, 2))
        want_pad = G.gcn_stack_forward(stack, xp, adj, in_width=323)[-1]
    with autograd_on():
        xr = x.clone().requires_grad_(True)
        got = [layer(xr, adj), layer(xr[0], adj), layer(xr, adj, ismlp=True), layer(xr, adj, relu=True), layer(xr, adj, ismlp=True, relu=True), nb(xr, adj)]
        got_stack = G.gcn_stack_forward(stack, xs.clone().requires_grad_(True), adj, keep=(0, 1, 2))
        got_nokeep = G.gcn_stack_forward(stack, xs.clone().requires_grad_(True), adj)
        got_pad = G.gcn_stack_forward(stack, xp.clone().requires_grad_(True), adj, in_width=323)[-1]
    for a, b in zip(want, got):
        assert b.requires_grad and torch.equal(a, b.detach())
    for a, b in zip(want_stack, got_stack):
        assert torch.equal(a, b.detach())
    assert got_nokeep[:3] == [None, None, None] and torch.equal(got_nokeep[3].detach(), want_stack[3])
    assert torch.equal(want_pad, got_pad.detach()) and torch.equal(want_pad, want_stack[3])


# ---- dW: the row-reduction GEMM -----------------------------------------------------------------------------------------------------------
def _check_gemm_tn(rng, rows, fin, cout, ldx=None, what=""):
    ldx = fin if ldx is None else ldx
    X = rng.standard_normal((rows, ldx)).astype(np.float32)
    dS = rng.standard_normal((rows, cout)).astype(np.float32)
    got = host(hip_gemm_tn(dev(X), fin, dev(dS)))
    x64, s64 = X[:, :fin].astype(np.float64), dS.astype(np.float64)
    assert_within(got, x64.T @ s64, rows, np.abs(x64).T @ np.abs(s64), f"dW rows={rows} {fin}->{cout} ldx={ldx} {what}")


@pytest.mark.parametrize("fin", [1, 3, 12, 195, 323, 128])
def test_gemm_tn_against_float64(fin):
    rng = np.random.default_rng(100 + fin)
    for cout in (1, 3, 16, 20, 128):
        for rows in row_counts(fin, cout):
            _check_gemm_tn(rng, rows, fin, cout)


@pytest.mark.parametrize("fin", [32, 33, 40, 70, 100, 129, 192, 193, 224, 225, 256, 300, 320, 321, 352, 353, 400])
def test_gemm_tn_other_widths(fin):
    """Widths outside the model's: every dispatch branch (128-feature blocks, 1 - 4 predicated tiles, both whole-row forms and their edges),
    a channel count with a ragged last tile (40) and one wider than four tiles (160)."""
    rng = np.random.default_rng(200 + fin)
    for cout in (40, 160):
        _check_gemm_tn(rng, 300, fin, cout)


def test_gemm_tn_row_stride_and_exact_placement():
    """ldx > Fin (the columns behind Fin hold garbage that must not be read into the sum), and an exact case: X = one-hot rows and integer dS,
    every partial sum an integer below 2^24, so dW must be the float64 product bit for bit -- a swapped row / column or a misplaced tile of
    the accumulator layout cannot hide behind a tolerance (asymmetric operands)."""
    rng = np.random.default_rng(7)
    for fin, cout in ((323, 128), (195, 20), (128, 3), (12, 20), (100, 40)):
        _check_gemm_tn(rng, 777, fin, cout, ldx=fin + 5, what="(strided)")
        rows = 1000
        X = np.zeros((rows, fin + 1), dtype=np.float32)
        X[np.arange(rows), rng.integers(0, fin, rows)] = 1.0
        X[:, fin] = 1e30
        dS = rng.integers(-8, 9, size=(rows, cout)).astype(np.float32)
        got = host(hip_gemm_tn(dev(X), fin, dev(dS)))
        assert np.array_equal(got, (X[:, :fin].astype(np.float64).T @ dS.astype(np.float64)).astype(np.float32)), (fin, cout)


def test_zero_rows_write_zeros():
    X, dS = torch.empty((0, 12), device="cuda"), torch.empty((0, 20), device="cuda")
    assert torch.equal(hip_gemm_tn(X, 12, dS), torch.zeros((12, 20), device="cuda"))
    assert torch.equal(hip_col_sum(dS, None), torch.zeros(20, device="cuda"))
    assert int(_lib.lib().g4d_gemm_tn_ws_bytes(0, 12, 20)) == 0


# ---- db ---------------------------------------------------------------------------------------------------------------------------------
def _masks(rng, shape):
    return {"none": None, "all zero": -np.ones(shape, np.float32), "all one": np.ones(shape, np.float32),
            "random": rng.standard_normal(shape).astype(np.float32)}


@pytest.mark.parametrize("c", [1, 3, 16, 20, 128, 300])
def test_col_sum_against_float64(c):
    rng = np.random.default_rng(300 + c)
    for rows in row_counts(128, c):
        dY = rng.standard_normal((rows, c)).astype(np.float32)
        for name, Y in _masks(rng, (rows, c)).items():
            got = host(hip_col_sum(dev(dY), None if Y is None else dev(Y)))
            g = dY.astype(np.float64) * (1.0 if Y is None else (Y > 0))
            assert_within(got, g.sum(0), rows, np.abs(g).sum(0), f"db rows={rows} c={c} mask {name}")
            if name == "all zero":
                assert not got.any()


# ---- dS ---------------------------------------------------------------------------------------------------------------------------------
def _check_spmm_grad(rng, adj, A, B, c):
    N = A.shape[0]
    dY = rng.standard_normal((B, N, c)).astype(np.float32)
    k = (A != 0).sum(0)[None, :, None]     # terms of dS[f, u, :] = entries of column u of A
    for name, Y in _masks(rng, (B, N, c)).items():
        got = host(hip_spmm_grad(dev(dY), None if Y is None else dev(Y), adj))
        g = dY.astype(np.float64) * (1.0 if Y is None else (Y > 0))
        ref = np.einsum("vu,fvc->fuc", A, g)
        assert_within(got, ref, k, np.einsum("vu,fvc->fuc", np.abs(A), np.abs(g)), f"dS B={B} N={N} c={c} mask {name}")
        if name == "all zero":
            assert not got.any()


@pytest.mark.parametrize("c", [1, 3, 16, 20, 128])
def test_spmm_rows_grad_against_float64(c):
    adj, A = fixture_adj()
    _check_spmm_grad(np.random.default_rng(400 + c), adj, A, 3, c)


def test_spmm_rows_grad_isolated_vertex_and_asymmetric_matrix():
    """A matrix with an empty row AND an empty column (an isolated vertex: zero dS row, no contribution), asymmetric values."""
    rng = np.random.default_rng(5)
    n = 37
    A = (rng.random((n, n)) < 0.15) * rng.standard_normal((n, n))
    A[11, :] = 0.0
    A[:, 11] = 0.0
    A[:, 20] = 0.0
    A = A.astype(np.float32)
    adj = sp.csr_matrix(A)
    for c in (3, 20, 128):
        _check_spmm_grad(rng, adj, A.astype(np.float64), 2, c)
    dY = dev(rng.standard_normal((2, n, 20)).astype(np.float32))
    dS = host(hip_spmm_grad(dY, None, adj))
    assert not dS[:, 11].any() and not dS[:, 20].any()


# ---- dX -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fin,cout", [(12, 20), (12, 3), (323, 128), (195, 128), (128, 128), (128, 3), (1, 1)])
def test_dx_contraction_against_float64(fin, cout):
    rng = np.random.default_rng(500 + fin + cout)
    layer = G.GraphConvolution(fin, cout).cuda()
    W = host(layer.weight).astype(np.float64)
    for rows in (1, 65, 1000):
        dS = rng.standard_normal((rows, cout)).astype(np.float32)
        got = host(fused.linear(dev(dS), layer._packed_transposed()))
        s64 = dS.astype(np.float64)
        assert got.shape == (rows, fin)
        assert_within(got, s64 @ W.T, cout, np.abs(s64) @ np.abs(W).T, f"dX rows={rows} {fin}<-{cout}")


# ---- full size ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_size():
    """240 frames x 4096 vertices, the first regressor layer (323 -> 128) with a fused ReLU: X, dY, Y on the device and one run of dS, dW, db."""
    _, faces = syn.quad_cylinder(64, 64)
    adj = G.adjacency_from_faces(faces, 4096)
    gen = torch.Generator(device="cuda").manual_seed(11)
    X = torch.randn((240 * 4096, 323), device="cuda", generator=gen)
    dY = torch.randn((240, 4096, 128), device="cuda", generator=gen)
    Y = torch.randn((240, 4096, 128), device="cuda", generator=gen)
    run = lambda: (hip_spmm_grad(dY, Y, adj), hip_col_sum(dY.view(-1, 128), Y.view(-1, 128)))
    dS, db = run()
    dW = hip_gemm_tn(X, 323, dS.view(-1, 128))
    torch.cuda.synchronize()
    return dict(adj=adj, X=X, dY=dY, Y=Y, dS=dS, dW=dW, db=db, run=run)


def test_full_size_dw_sample_and_db_against_float64(full_size):
    """983 040 rows: 16 feature rows of dW (2048 elements, ragged last tile included) and all of db, float64 accumulated over row chunks."""
    fs = full_size
    rows = fs["X"].shape[0]
    cols = np.array([0, 1, 2, 3, 127, 128, 129, 200, 255, 256, 257, 319, 320, 321, 322, 64])
    ct = torch.from_numpy(cols).cuda()
    dW = np.zeros((16, 128)); aW = np.zeros((16, 128)); db = np.zeros(128); ab = np.zeros(128)
    dY2, Y2, dS2 = fs["dY"].view(-1, 128), fs["Y"].view(-1, 128), fs["dS"].view(-1, 128)
    for r0 in range(0, rows, 1 << 16):
        sl = slice(r0, min(rows, r0 + (1 << 16)))
        x = host(fs["X"][sl][:, ct]).astype(np.float64)
        s = host(dS2[sl]).astype(np.float64)
        g = host(dY2[sl]).astype(np.float64) * (host(Y2[sl]) > 0)
        dW += x.T @ s; aW += np.abs(x).T @ np.abs(s); db += g.sum(0); ab += np.abs(g).sum(0)
    assert_within(host(fs["dW"])[cols], dW, rows, aW, "full-size dW sample")
    assert_within(host(fs["db"]), db, rows, ab, "full-size db")


def test_full_size_is_deterministic(full_size):
    fs = full_size
    dS, db = fs["run"]()
    dW = hip_gemm_tn(fs["X"], 323, dS.view(-1, 128))
    assert torch.equal(dS, fs["dS"]) and torch.equal(db, fs["db"]) and torch.equal(dW, fs["dW"])
    assert not torch.isnan(dW).any() and not torch.isnan(dS).any()


# ---- the reference's autograd -------------------------------------------------------------------------------------------------------------
def _gate(name, got, ref64, e_ref, k, abs_sum):
    """>= 1024 elements: max |hip - ref64| <= 3 e_ref; fewer: every element within the derived bound of its last summation."""
    got = got.astype(np.float64)
    assert got.shape == ref64.shape, name
    err = float(np.abs(got - ref64).max())
    print(f"{name}: max |hip - ref64| = {err:.3e}, e_ref = {e_ref:.3e}, ratio {err / e_ref if e_ref else float('nan'):.3f}, elements {got.size}")
    if got.size >= 1024:
        assert err <= 3 * e_ref, f"{name}: max |hip - ref64| = {err:.3e} > 3 x e_ref = {3 * e_ref:.3e}"
    else:
        assert_within(got, ref64, k, abs_sum, name)


def test_single_layers_against_the_reference_autograd():
    """Every stored gradient of the four single-layer cases.  Measured on MI355X, max |hip - ref64| / e_ref of the tensors the 3 e_ref gate
    applies to: l3d dx 0.99, mlp dx 1.26, nb dx 1.00.  The others (< 1024 elements, derived bound; worst err / bound 0.08): l2d dx 0.75, dW
    1.00 in all four cases, db 1.15 / 1.92 (l2d) / 1.15."""
    g, o = TW.load()
    adj, A = fixture_adj()
    for name, ismlp in (("l3d", False), ("l2d", False), ("mlp", True), ("nb", False)):
        has_b = f"{name}_b" in g.files
        layer = G.GraphConvolution(12, g[f"{name}_W"].shape[1], bias=has_b).cuda()
        layer.weight.data = dev(g[f"{name}_W"])
        if has_b:
            layer.bias.data = dev(g[f"{name}_b"])
        x = dev(g[f"{name}_x"]).requires_grad_(True)
        with autograd_on():
            y = layer(x, adj, ismlp=ismlp)
        y.backward(dev(g[f"{name}_dy"]))
        dy64 = g[f"{name}_dy"].astype(np.float64)
        _, _, _, _, ab = TW.layer_backward(g[f"{name}_x"], g[f"{name}_W"], A, dy64, ismlp=ismlp, need_abs=True)
        rows = int(np.prod(dy64.shape[:-1]))
        got = {"dx": x.grad, "dW": layer.weight.grad, "db": layer.bias.grad if has_b else None}
        for k, kk in (("dx", dy64.shape[-1]), ("dW", rows), ("db", rows)):
            if got[k] is None:
                continue
            ref64, ref32 = g[f"{name}_{k}64"], g[f"{name}_{k}"]
            _gate(f"{name}_{k}", host(got[k]), ref64, float(np.abs(ref32 - ref64).max()), kk, ab[k])


def test_stack_against_the_reference_autograd():
    """The regressor 323 -> 128 -> 128 -> 128 -> 3 through gcn_stack_forward: dx and all eight parameter gradients.  ref64 = the float64 twin
    (tests/test_gcn_grad_cpu.py ties it to the reference's float64 run), e_ref from the file.  No element is masked: the fixture's smallest
    hidden |pre-activation| is asserted >= 2e-5.  Measured on MI355X, max |hip - ref64| / e_ref of the tensors the 3 e_ref gate applies to:
    dx 1.06, dW0 1.20, dW1 1.16, dW2 0.76.  The others (< 1024 elements, derived bound; worst err / bound 0.64 at dW3): dW3 1.22,
    db0..3 0.92 / 1.19 / 0.81 / 1.62."""
    g, o = TW.load()
    adj, A = fixture_adj()
    assert float(g["stack_min_preact"]) >= 2e-5
    layers = [G.GraphConvolution(a, b).cuda() for a, b in zip(TW.WIDTHS[:-1], TW.WIDTHS[1:])]
    for i, m in enumerate(layers):
        m.weight.data, m.bias.data = dev(g[f"stack_W{i}"]), dev(g[f"stack_b{i}"])
    x = dev(g["stack_x"]).requires_grad_(True)
    with autograd_on():
        y = G.gcn_stack_forward(layers, x, adj)[-1]
    y.backward(dev(g["stack_dy"]))
    grads, pres, ab = TW.stack_grads(g["stack_x"], [g[f"stack_W{i}"] for i in range(4)], [g[f"stack_b{i}"] for i in range(4)], A, g["stack_dy"],
                                     need_abs=True)
    got = {"dx": x.grad}
    for i, m in enumerate(layers):
        got[f"dW{i}"], got[f"db{i}"] = m.weight.grad, m.bias.grad
    for k, ref64 in grads.items():
        kk = TW.WIDTHS[1] if k == "dx" else 128    # terms of the last summation: Cout of layer 0 for dx, B x Vg = 128 rows for dW / db
        _gate(f"stack_{k}", host(got[k]), ref64, float(g[f"stack_eref_{k}"]), kk, ab[k])


# ---- padding, skipped launches ---------------------------------------------------------------------------------------------------------------
def test_in_width_padding_gives_the_same_gradients():
    adj, _ = fixture_adj()
    torch.manual_seed(9)
    layers = [G.GraphConvolution(a, b).cuda() for a, b in zip(TW.WIDTHS[:-1], TW.WIDTHS[1:])]
    xs = torch.randn(2, 64, 323, device="cuda")
    xp = torch.zeros(2, 64, 324, device="cuda")
    xp[..., :323] = xs
    dy = torch.randn(2, 64, 3, device="cuda")
    res = []
    for x, kw in ((xs, {}), (xp, dict(in_width=323))):
        for m in layers:
            m.weight.grad = m.bias.grad = None
        x = x.clone().requires_grad_(True)
        with autograd_on():
            G.gcn_stack_forward(layers, x, adj, **kw)[-1].backward(dy)
        res.append((x.grad, [m.weight.grad for m in layers], [m.bias.grad for m in layers]))
    (gx, gw, gb), (px, pw, pb) = res
    assert px.shape == (2, 64, 324) and torch.equal(px[..., :323], gx) and not px[..., 323:].any()
    assert pw[0].shape == (323, 128)
    assert all(torch.equal(a, b) for a, b in zip(gw, pw)) and all(torch.equal(a, b) for a, b in zip(gb, pb))


def test_needs_input_grad_skips_launches(monkeypatch):
    adj, _ = fixture_adj()
    layer = G.GraphConvolution(12, 20).cuda()
    calls = []
    real = _lib.call

    def counting(name, *a):
        calls.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", counting)
    contractions = {"g4d_linear_f32", "g4d_mlp_run"}
    # (a) the input needs no gradient (the first layer of a stack): no dX contraction
    x = torch.randn(3, 64, 12, device="cuda")
    with autograd_on():
        y = layer(x, adj)
    calls.clear()
    y.sum().backward()
    assert set(calls) == {"g4d_spmm_rows_grad_f32", "g4d_col_sum_rows_f32", "g4d_gemm_tn_f32"} and not contractions & set(calls), calls
    assert layer.weight.grad is not None and layer.bias.grad is not None
    # (b) frozen parameters: no dW, no db
    layer.weight.grad = layer.bias.grad = None
    layer.weight.requires_grad_(False); layer.bias.requires_grad_(False)
    x = x.clone().requires_grad_(True)
    with autograd_on():
        y = layer(x, adj)
    calls.clear()
    y.sum().backward()
    assert "g4d_gemm_tn_f32" not in calls and "g4d_col_sum_rows_f32" not in calls and "g4d_spmm_rows_grad_f32" in calls, calls
    assert contractions & set(calls) and layer.weight.grad is None and layer.bias.grad is None and x.grad is not None
    # (c) frozen weight, trainable bias, an input without gradient: the column sums alone
    layer.bias.requires_grad_(True)
    with autograd_on():
        y = layer(x.detach(), adj)
    calls.clear()
    y.sum().backward()
    assert calls == ["g4d_col_sum_rows_f32"], calls
    assert layer.bias.grad is not None and layer.weight.grad is None


def test_relu_extension_and_2d_input_gradients():
    """relu=True (mask from the saved output), ismlp + relu, and a 2-D input, against the float64 twin with the derived bounds."""
    g, o = TW.load()
    adj, A = fixture_adj()
    layer = G.GraphConvolution(12, 20).cuda()
    layer.weight.data, layer.bias.data = dev(g["l3d_W"]), dev(g["l3d_b"])
    for xn, ismlp in ((g["l3d_x"], False), (g["l3d_x"], True), (g["l2d_x"], False)):
        dyn = g["l3d_dy"] if xn.ndim == 3 else g["l2d_dy"]
        x = dev(xn).requires_grad_(True)
        layer.weight.grad = layer.bias.grad = None
        with autograd_on():
            y = layer(x, adj, ismlp=ismlp, relu=True)
        y.backward(dev(dyn))
        pre = TW.layer_forward(xn, g["l3d_W"], g["l3d_b"], A, ismlp=ismlp)
        # the mask the kernels see is the one of the HIP forward's own output; it must be the float64 one wherever the pre-activation is
        # further from zero than the forward's own rounding bound (contraction of 12 terms, aggregation of <= 5, bias)
        mask = host(y) > 0
        a64, x64, w64 = np.abs(A), np.abs(xn.astype(np.float64)), np.abs(g["l3d_W"].astype(np.float64))
        fwd_abs = (x64 @ w64 if ismlp else np.einsum("vu,...uc->...vc", a64, x64 @ w64)) + np.abs(g["l3d_b"].astype(np.float64))
        sure = np.abs(pre) > TW.sum_bound(12 + 5 + 1, fwd_abs)
        assert sure.mean() > 0.99 and np.array_equal(mask[sure], (pre > 0)[sure])
        gm = dyn.astype(np.float64) * mask
        dx, dW, db, _, ab = TW.layer_backward(xn, g["l3d_W"], A, gm, ismlp=ismlp, need_abs=True)
        rows = int(np.prod(gm.shape[:-1]))
        # dX and dW sum over dS, itself an fp32 sum of kin <= 5 terms (0 with ismlp: dS = G exactly): the composed double sum has
        # kin + k terms' worth of roundings over the NESTED sum of |term| (|A|^T |G| in place of |dS|)
        kin = 0 if ismlp else int((A != 0).sum(0).max()) + 2
        a_ds = ab["ds"]
        assert_within(host(x.grad), dx, 20 + kin, a_ds @ np.abs(g["l3d_W"].astype(np.float64)).T, f"relu dx ismlp={ismlp} ndim={xn.ndim}")
        assert_within(host(layer.weight.grad), dW, rows + kin, np.abs(xn.astype(np.float64)).reshape(rows, -1).T @ a_ds.reshape(rows, -1),
                      f"relu dW ismlp={ismlp} ndim={xn.ndim}")
        assert_within(host(layer.bias.grad), db, rows, ab["db"], f"relu db ismlp={ismlp} ndim={xn.ndim}")
