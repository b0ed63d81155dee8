"""The adjoint of the garment skinning on HIP (csrc/skin/skin_grad.hip, include/g4d_skin.h) behind tuning.Tuning.garment_lbs_autograd: each entry
point alone against the float64 numpy twin (tests/garment_skin_grad_twin.py) over its launch edges, the whole autograd node against the twin and
against the reference's own autograd (tests/golden/garment_skin_grad.npz), and the exact properties (same bits on every run, a clip's bits
independent of the batch, a NaN clip stays alone, the zero rule at a coincident vertex, refusals, hipGraph replay).
The gate everywhere: max |got - float64| <= 3 x max |fp32 torch autograd of the twin's restatement - float64| on the same inputs (the measure of
tests/test_smpl_grad_gpu.py); against the golden, 3 x the reference's own fp32-vs-float64 error."""
import functools

import numpy as np
import pytest
import torch

import garment_skin_grad_twin as GT
from conftest import load_golden
from garment4d_amd import _lib, garment_lbs as GL, gcn, grad_ops, synthetic as syn, tuning

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
PAD = 67


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _on():
    return tuning.use(tuning.current().replace(garment_lbs_autograd=True))


def _padded(shape):
    """An output buffer with PAD sentinel floats behind it: (flat buffer, view of the output)."""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[:n].view(shape)


def _gate(tag, got, want, t32, failures):
    err, eref = np.abs(got.astype(np.float64) - want).max(), np.abs(t32 - want).max()
    print(f"{tag}: max |err| {err:.3e}  torch fp32 {eref:.3e}  err / (3 torch) {err / (3 * eref) if eref else (0.0 if err == 0 else float('inf')):.3f}  (max |grad| {np.abs(want).max():.3e})")
    if not err <= 3 * eref:
        failures.append((tag, err, eref))


# ------------------------------------------------------------------------------------------------------------------------- g4d_garment_skin_grad_f32
#              clips T  Vg   J   per_clip outputs
SKIN_SWEEP = [(1,   1, 1,   24, False, "both"),
              (2,   3, 63,  5,  False, "both"),
              (2,   3, 65,  24, True,  "both"),
              (1,   3, 192, 24, False, "verts"),
              (2,   1, 192, 5,  False, "W"),
              (2,   3, 257, 24, False, "both"),      # a second block along the vertices
              (1,   3, 65,  5,  True,  "W"),
              (2,   3, 63,  32, True,  "both"),      # the 32- and 64-joint register forms
              (1,   3, 65,  40, False, "both")]


@functools.lru_cache(maxsize=None)
def _skin_case(clips, T, Vg, J, per_clip):
    rng = np.random.default_rng(clips * 1000 + T * 100 + Vg + J)
    F_ = clips * T
    W = rng.random((clips if per_clip else F_, Vg, J)) ** 3 + 1e-3
    W = (W / W.sum(-1, keepdims=True)).astype(np.float32)
    A = (np.tile(np.eye(4), (F_, J, 1, 1)) + 0.3 * rng.standard_normal((F_, J, 4, 4))).astype(np.float32)
    verts = (rng.standard_normal((clips, Vg, 3)) * 0.4).astype(np.float32)
    d_out, d_add = rng.standard_normal((F_, Vg, 3)).astype(np.float32), rng.standard_normal((clips, Vg, 3)).astype(np.float32)
    f64 = lambda a: a.astype(np.float64)
    want = GT.skin_grad(f64(W), f64(A), f64(verts), f64(d_out), T)
    # fp32 torch autograd of the restatement
    Wt, vt = torch.from_numpy(W).requires_grad_(True), torch.from_numpy(verts).requires_grad_(True)
    cl = torch.arange(F_) // T
    Tm = torch.einsum("fvj,fjrc->fvrc", Wt[cl] if per_clip and T > 1 else Wt, torch.from_numpy(A)[:, :, :3, :])
    y = torch.einsum("fvrc,fvc->fvr", Tm[..., :3], vt[cl]) + Tm[..., 3]
    (y * torch.from_numpy(d_out)).sum().backward()
    return W, A, verts, d_out, d_add, want, (vt.grad.double().numpy(), Wt.grad.double().numpy())


@pytest.mark.parametrize("clips,T,Vg,J,per_clip,outputs", SKIN_SWEEP)
def test_skin_adjoint_matches_the_twin_and_writes_nothing_else(clips, T, Vg, J, per_clip, outputs):
    W, A, verts, d_out, d_add, want, t32 = _skin_case(clips, T, Vg, J, per_clip)
    _lib.skin_lib()
    Wd, Ad, vd, gd, addd = _dev(W), _dev(A), _dev(verts), _dev(d_out), _dev(d_add)
    vbuf, dv = _padded((clips, Vg, 3))
    wbuf, dW = _padded(W.shape)
    _lib.call("g4d_garment_skin_grad_f32", clips, T, Vg, J, Wd.data_ptr(), int(per_clip and T > 1), Ad.data_ptr(), vd.data_ptr(), gd.data_ptr(), addd.data_ptr(),
              dv.data_ptr() if outputs != "W" else 0, dW.data_ptr() if outputs != "verts" else 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (vbuf[dv.numel():] == SENTINEL).all() and (wbuf[dW.numel():] == SENTINEL).all()
    failures = []
    if outputs != "W":
        _gate(f"skin {(clips, T, Vg, J, per_clip)} d_verts", dv.cpu().numpy() - d_add.astype(np.float64), want[0], t32[0], failures)
        # ... and d_add is ADDED, exactly: the call without it gives the same sum
        dv0 = grad_ops.garment_skin_grad(clips, T, Wd, Ad, vd, gd, want_W=False)[0]
        assert torch.equal(dv, addd + dv0)
    else:
        assert (vbuf == SENTINEL).all()                                     # a NULL output is not written
    if outputs != "verts":
        _gate(f"skin {(clips, T, Vg, J, per_clip)} d_W", dW.cpu().numpy(), want[1], t32[1], failures)
    else:
        assert (wbuf == SENTINEL).all()
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------------- g4d_knn_blend_grad_f32
V = 300
#               clips T  Vg   K    J   per_clip ldk
BLEND_SWEEP = [(1,   1, 1,   1,   24, False, 1),
               (2,   3, 63,  3,   5,  False, 3),
               (2,   3, 65,  63,  24, True,  63),
               (1,   3, 192, 64,  24, False, 64),
               (2,   1, 65,  65,  5,  False, 65),
               (2,   3, 63,  256, 24, False, 256),
               (1,   3, 65,  256, 5,  True,  256),
               (2,   3, 1,   64,  24, False, 256),    # the prefix of a longer list (the un-posing's blend)
               (2,   1, 192, 3,   24, False, 70),
               (1,   1, 63,  1,   5,  False, 1),
               (2,   3, 65,  130, 24, True,  130)]     # three 64-lane chunks, the last one partial


@functools.lru_cache(maxsize=None)
def _blend_case(clips, T, Vg, K, J, per_clip, ldk, coincident=False):
    rng = np.random.default_rng(clips * 1000 + T * 100 + Vg + K + J + ldk)
    F_ = clips if per_clip else clips * T
    fpc = 1 if per_clip else T
    tab = rng.random((F_, V, J)) ** 3 + 1e-3
    tab = (tab / tab.sum(-1, keepdims=True)).astype(np.float32)
    pts, ref = (rng.standard_normal((clips, Vg, 3)) * 0.3).astype(np.float32), (rng.standard_normal((clips, V, 3)) * 0.3).astype(np.float32)
    d2 = ((pts[:, :, None].astype(np.float64) - ref[:, None]) ** 2).sum(-1)
    idx = np.argsort(d2, axis=-1, kind="stable")[..., :ldk].astype(np.int32)
    if coincident:
        pts[0, min(3, Vg - 1)] = ref[0, idx[0, min(3, Vg - 1), 0]]
    nb = ref[np.arange(clips)[:, None, None], idx]
    diff = pts[:, :, None] - nb
    dists = ((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]).astype(np.float32)   # fp32, as a KNN hands them over
    d_blend = rng.standard_normal((F_, Vg, J)).astype(np.float32)
    d_add = rng.standard_normal((clips, Vg, 3)).astype(np.float32)
    f64 = lambda a: a.astype(np.float64)
    want = GT.blend_grad(f64(tab), fpc, idx[..., :K], f64(dists[..., :K]), f64(d_blend), f64(pts), f64(ref))
    # fp32 torch autograd of the restatement: distances from the points, reciprocal, masked assignment, gather, weighted sum
    pt = torch.from_numpy(pts).requires_grad_(True)
    it = torch.from_numpy(idx[..., :K].astype(np.int64))
    d = ((pt[:, :, None] - torch.from_numpy(ref)[torch.arange(clips)[:, None, None], it]) ** 2).sum(-1)
    r = 1.0 / d
    r = torch.where(torch.isinf(r), torch.zeros_like(r), r)
    w = r / r.sum(-1, keepdim=True)
    w = torch.where(torch.isinf(w), torch.zeros_like(w), w)
    cl = torch.arange(F_) // fpc
    out = (torch.from_numpy(tab)[torch.arange(F_)[:, None, None], it[cl]] * w[cl][..., None]).sum(-2)
    (out * torch.from_numpy(d_blend)).sum().backward()
    return tab, fpc, idx, dists, d_blend, pts, ref, d_add, want, pt.grad.double().numpy()


def _run_blend(case, K, d_add=None, out=None):
    tab, fpc, idx, dists, d_blend, pts, ref = case[:7]
    clips, Vg, ldk = idx.shape
    _lib.skin_lib()
    keep = [_dev(tab), _dev(idx, np.int32), _dev(dists), _dev(d_blend), _dev(pts), _dev(ref)]
    out = torch.empty((clips, Vg, 3), dtype=torch.float32, device="cuda") if out is None else out
    _lib.call("g4d_knn_blend_grad_f32", tab.shape[0], fpc, Vg, V, K, ldk, tab.shape[2], *[t.data_ptr() for t in keep], 0 if d_add is None else d_add.data_ptr(),
              out.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("clips,T,Vg,K,J,per_clip,ldk", BLEND_SWEEP)
def test_blend_adjoint_matches_the_twin_and_writes_nothing_else(clips, T, Vg, K, J, per_clip, ldk):
    case = _blend_case(clips, T, Vg, K, J, per_clip, ldk)
    want, t32, d_add = case[8], case[9], case[7]
    buf, out = _padded((clips, Vg, 3))
    _run_blend(case, K, out=out)
    assert (buf[out.numel():] == SENTINEL).all()
    failures = []
    _gate(f"blend {(clips, T, Vg, K, J, per_clip, ldk)} d_pts", out.cpu().numpy(), want, t32, failures)
    assert not failures, failures
    if K == 1:
        assert (out == 0).all()                                             # one neighbour has weight 1 whatever its distance: exactly zero
    addd = _dev(d_add)
    assert torch.equal(_run_blend(case, K, d_add=addd), addd + out)          # d_add is added, exactly
    inplace = addd.clone()
    assert torch.equal(_run_blend(case, K, d_add=inplace, out=inplace), addd + out)   # ... also in place


def test_two_runs_give_equal_bits_and_a_clips_bits_do_not_depend_on_its_batch():
    case = _blend_case(2, 3, 65, 130, 24, False, 130)
    a, b = _run_blend(case, 130), _run_blend(case, 130)
    assert np.array_equal(_bits(a), _bits(b))
    tab, fpc, idx, dists, d_blend, pts, ref = case[:7]
    for c in (0, 1):
        one = (tab[c * 3:c * 3 + 3], fpc, idx[c:c + 1], dists[c:c + 1], d_blend[c * 3:c * 3 + 3], pts[c:c + 1], ref[c:c + 1])
        assert np.array_equal(_bits(_run_blend(one, 130))[0], _bits(a)[c]), c
    W, A, verts, d_out, d_add, _, _ = _skin_case(2, 3, 65, 24, True)
    run = lambda sl_c, sl_f: grad_ops.garment_skin_grad(sl_c.stop - sl_c.start, 3, _dev(W[sl_c]), _dev(A[sl_f]), _dev(verts[sl_c]), _dev(d_out[sl_f]))
    full, again = run(slice(0, 2), slice(0, 6)), run(slice(0, 2), slice(0, 6))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(full, again))
    for c in (0, 1):
        one = run(slice(c, c + 1), slice(3 * c, 3 * c + 3))
        assert np.array_equal(_bits(one[0])[0], _bits(full[0])[c]) and np.array_equal(_bits(one[1])[0], _bits(full[1])[c]), c


def test_a_nan_clip_stays_alone():
    case = list(_blend_case(2, 3, 65, 130, 24, False, 130))
    good = _run_blend(case, 130)
    case[4], case[5] = case[4].copy(), case[5].copy()
    case[4][3:] = np.nan                                                    # clip 1's upstream gradient and points
    case[5][1] = np.nan
    bad = _run_blend(case, 130)
    assert np.array_equal(_bits(bad)[0], _bits(good)[0]) and torch.isnan(bad[1]).all()
    W, A, verts, d_out, _, _, _ = _skin_case(2, 3, 65, 24, True)
    ok = grad_ops.garment_skin_grad(2, 3, _dev(W), _dev(A), _dev(verts), _dev(d_out))
    A2 = A.copy()
    A2[4] = np.nan                                                          # one frame of clip 1
    nan = grad_ops.garment_skin_grad(2, 3, _dev(W), _dev(A2), _dev(verts), _dev(d_out))
    assert all(np.array_equal(_bits(x)[0], _bits(y)[0]) for x, y in zip(ok, nan)) and torch.isnan(nan[0][1]).all()


def test_a_coincident_vertex_gets_the_twins_finite_gradient():
    """Garment vertex (0, 3) lies exactly on its nearest body vertex (d_0 = 0 in the list handed over): torch autograd gives NaN there; the kernel
    gives the twin's finite value.  The bound is 3 x the fp32 autograd error over the vertices where autograd is finite."""
    case = _blend_case(2, 3, 65, 63, 24, False, 63, True)
    dists, want, t32 = case[3], case[8], case[9]
    assert dists[0, 3, 0] == 0 and (dists[0, 3, 1:] > 0).all() and np.isnan(t32[0, 3]).all() and np.isfinite(want).all()
    got = _run_blend(case, 63).cpu().numpy()
    fin = np.isfinite(t32)
    eref = np.abs(t32[fin] - want[fin]).max()
    err = np.abs(got - want).max()
    print(f"coincident vertex: max |err| {err:.3e} (at the vertex {np.abs(got[0, 3] - want[0, 3]).max():.3e})  torch fp32 elsewhere {eref:.3e}  ratio {err / (3 * eref):.3f}")
    assert np.isfinite(got).all() and err <= 3 * eref


def test_both_calls_replayed_from_a_hip_graph_give_the_eager_bits():
    """skin adjoint -> blend adjoint (its d_W is the blend's d_blend, its d_verts the blend's d_add): a linear chain of two launches."""
    W, A, verts, d_out, _, _, _ = _skin_case(2, 3, 65, 24, False)
    tab, fpc, idx, dists, _, pts, ref = _blend_case(2, 3, 65, 63, 24, False, 63)[:7]
    Wd, Ad, vd, gd, tabd, idxd, dd, pd, rd = _dev(W), _dev(A), _dev(verts), _dev(d_out), _dev(tab), _dev(idx, np.int32), _dev(dists), _dev(pts), _dev(ref)

    def chain():
        dv, dW = grad_ops.garment_skin_grad(2, 3, Wd, Ad, vd, gd)
        return grad_ops.knn_blend_grad(tabd, fpc, idxd, dd, 63, dW, pd, rd, d_add=dv)
    eager = chain()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        chain()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain()
    for _ in range(2):
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), _bits(eager))


# ------------------------------------------------------------------------------------------------------------------------- the whole Function
@functools.lru_cache(maxsize=None)
def _scene():
    sc = syn.garment_scene(2, 3, 4, body_rc=(15, 20), garment_rc=(8, 8), seed=11)
    rng = np.random.default_rng(12)
    W = sc["batch"]["T_lbs_weights"] * (1 + 0.2 * rng.random(sc["batch"]["T_lbs_weights"].shape))     # per-frame tables that differ
    sc["batch"]["T_lbs_weights"] = (W / W.sum(-1, keepdims=True)).astype(np.float32)
    gv, gq = sc["template"]
    x = (gv[None] + rng.standard_normal((2,) + gv.shape) * 0.004).astype(np.float32)
    return sc, x, gcn.adjacency_old_from_faces(gq, gv.shape[0])


def _call(x, K, shared, sc, adj_old, **kw):
    b = {k: _dev(v) for k, v in sc["batch"].items()}
    b.update(kw)
    Jr, W = b["T_J_regressor"], b["T_lbs_weights"]
    if shared:
        Jr, W = Jr[:, :1].expand(-1, 3, -1, -1), W[:, :1].expand(-1, 3, -1, -1)
        assert W.stride(1) == 0
    return GL.lbs_garment_interpolation(x, b["Tpose_smpl_vertices_torch"], b["Tpose_smpl_root_joints_torch"], b["zeropose_smpl_vertices_torch"],
                                        torch.from_numpy(sc["body"]["parents"]).cuda(), b["pose_torch"], Jr, W, adj_old, K=K)


@pytest.mark.parametrize("K,shared", [(1, False), (3, False), (3, True), (70, False), (256, True), (256, False)])
def test_function_forward_bits_and_gradients_alone_and_together(K, shared):
    """Under the flag the forward has the flag-off call's bits; posed.backward, the un-posed output's gradient, and both, against the twin given
    the node's own neighbour lists and fp32 transforms."""
    sc, x, adj_old = _scene()
    assert sc["batch"]["T_lbs_weights"].shape[2] == 300
    with torch.no_grad():
        p0, n0, s0 = _call(_dev(x), K, shared, sc, adj_old)
    xr = _dev(x).requires_grad_(True)
    off = _call(xr, K, shared, sc, adj_old)
    assert off[0].grad_fn is None and off[2].grad_fn is None                 # flag off: no graph, as ever
    with _on():
        posed, nn1, stage1 = _call(xr, K, shared, sc, adj_old)
    assert posed.grad_fn is not None and stage1.grad_fn is not None and not nn1.dists.requires_grad and nn1.idx.dtype == torch.long
    assert np.array_equal(_bits(posed), _bits(p0)) and np.array_equal(_bits(stage1), _bits(s0)) and torch.equal(nn1.idx, n0.idx) and torch.equal(nn1.dists, n0.dists)
    node = posed.grad_fn
    g, body, idx_k, d_k, cW, inv_nn_W, inv_A, u, Wt, nn_W, A = node.saved_tensors
    assert Wt.shape[0] == (2 if shared else 6) and nn_W.shape[0] == Wt.shape[0] and idx_k.shape == (2, 64, K)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    c = dict(root=sc["batch"]["Tpose_smpl_root_joints_torch"].reshape(2, 3).astype(np.float64), body=f64(body), idx=idx_k.cpu().numpy(), cW=f64(cW), Wt=f64(Wt),
             inv_A=f64(inv_A), A=f64(A), M=GT.step_operator(adj_old), iters=100)
    rng = np.random.default_rng(13)
    dy, ds = rng.standard_normal((2, 3, 64, 3)).astype(np.float32), rng.standard_normal((2, 3, 64, 3)).astype(np.float32)
    failures = []
    for name, use_y, use_s in (("posed", True, False), ("un-posed", False, True), ("both", True, True)):
        xr.grad = None
        loss = ((posed * _dev(dy)).sum() if use_y else 0) + ((stage1 * _dev(ds)).sum() if use_s else 0)
        loss.backward(retain_graph=True)
        a, b = (dy.reshape(6, 64, 3).astype(np.float64) if use_y else None), (ds.astype(np.float64).sum(1) if use_s else None)
        want = GT.adjoint(x.astype(np.float64), c, a, b)
        t32 = GT.torch_grad(x, c, None if a is None else a.astype(np.float32), None if b is None else b.astype(np.float32), torch.float32)
        _gate(f"function K={K} shared={shared} {name}", xr.grad.cpu().numpy(), want, t32, failures)
    assert not failures, failures


@pytest.mark.parametrize("K", [3, 256])
def test_function_matches_the_references_autograd_within_three_times_its_own_fp32_error(K):
    g = load_golden("garment_skin_grad.npz")
    case = GT.golden_case()
    b = {k: _dev(v) for k, v in case["batch"].items()}
    adj_old = gcn.adjacency_old_from_faces(case["template_faces"], case["Vg"])
    x = _dev(case["tpose_garment"]).requires_grad_(True)
    with _on():
        posed, _, stage1 = GL.lbs_garment_interpolation(x, b["Tpose_smpl_vertices_torch"], b["Tpose_smpl_root_joints_torch"], b["zeropose_smpl_vertices_torch"],
                                                        torch.from_numpy(case["body"]["parents"]).cuda(), b["pose_torch"], b["T_J_regressor"], b["T_lbs_weights"],
                                                        adj_old, K=K)
    assert np.array_equal(posed.grad_fn.saved_tensors[2].cpu().numpy(), g[f"k{K}_idx"].astype(np.int32))     # the lists the reference differentiated at
    failures = []
    for name in ("posed", "both"):
        x.grad = None
        loss = (posed * _dev(case["dy"])).sum() + ((stage1 * _dev(case["ds"])).sum() if name == "both" else 0)
        loss.backward(retain_graph=True)
        want, eref = g[f"k{K}_{name}_dx32"], float(g[f"k{K}_{name}_eref"])
        err = np.abs(x.grad.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max()
        err64 = np.abs(x.grad.cpu().numpy().astype(np.float64) - g[f"k{K}_{name}_dx64"]).max()
        print(f"golden K={K} {name}: max |err| vs the reference's fp32 {err:.3e} (vs its float64 {err64:.3e})  eref {eref:.3e}  err / (3 eref) {err / (3 * eref):.3f}")
        if not err <= 3 * eref:
            failures.append((name, err, eref))
    assert not failures, failures


def test_a_grad_requiring_body_or_pose_is_refused_under_the_flag():
    sc, x, adj_old = _scene()
    xr = _dev(x).requires_grad_(True)
    with _on():
        for key in ("Tpose_smpl_vertices_torch", "pose_torch", "T_lbs_weights"):
            with pytest.raises(NotImplementedError, match=r"only pred_template_garment_v is differentiated"):
                _call(xr, 3, False, sc, adj_old, **{key: _dev(sc["batch"][key]).requires_grad_(True)})
        with torch.no_grad():
            assert _call(xr, 3, False, sc, adj_old)[0].grad_fn is None
