"""The MGN training route on the GPU: g4d_mgn_skin_grad_f32 against the float64 twin (tests/mgn_grad_twin.py) within its derived bound and against
the forward kernel through the adjoint identity, its argument checks and index clamp, the displacement MLP's Linear nodes against torch-float64
autograd of the same layers, and the model (PCALBSGarmentUseSegEncoderSegMGN.forward under tuning.Tuning.mgn_autograd) against the reference's
own training step (tests/golden/mgn_grad.npz)."""
import types

import numpy as np
import pytest
import torch

import mgn_grad_twin as MT
import stage2_loss_twin as TW
from garment4d_amd import _cache, _lib, grad_ops, losses, tuning
from garment4d_amd import lbs as L
from garment4d_amd import synthetic as syn
from garment4d_amd.garment_lbs import lbs_garment_MGN
from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSegMGN, _LinearFn

pytestmark = pytest.mark.gpu

LOSS_CFG = dict(zip(losses.LOSS_LAMBDAS, TW.LAMBDAS))
def on():
    return tuning.use(tuning.current().replace(mgn_autograd=True))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _transforms(F_, J, seed):
    """(F,J,4,4) rigid joint transforms from the lbs helpers: random axis-angle poses about random joints."""
    rng = np.random.default_rng(seed)
    parents = syn.SMPL_PARENTS if J == 24 else np.array([-1] + [int(rng.integers(0, i)) for i in range(1, J)], dtype=np.int64)
    rot = L.batch_rodrigues(dev((rng.standard_normal((F_ * J, 3)) * 0.3).astype(np.float32))).reshape(F_, J, 3, 3)
    joints = dev((rng.standard_normal((F_, J, 3)) * 0.3).astype(np.float32))
    return L.batch_rigid_transform(rot, joints, parents)[1].contiguous()


def _weights(F_, V, J, seed):
    rng = np.random.default_rng(seed)
    w = rng.random((F_, V, J)).astype(np.float32) ** 4
    return dev((w / w.sum(-1, keepdims=True)).astype(np.float32))


def _grad(clips, T, idx, W, inv_A, A, dp, ds=None):
    """g4d_mgn_skin_grad_f32 into a NaN-filled buffer."""
    F_, Vg = idx.shape[:2]
    out = torch.full((F_, Vg, 3), float("nan"), dtype=torch.float32, device="cuda")
    _lib.call("g4d_mgn_skin_grad_f32", clips, T, Vg, W.shape[1], W.shape[2], idx.data_ptr(), W.data_ptr(), inv_A.data_ptr(), A.data_ptr(), dp.data_ptr(),
              0 if ds is None else ds.data_ptr(), out.data_ptr(), _lib.stream_ptr())
    return out


# (clips, frames_per_clip, Vg, V, J): the smallest sizes; V = 1; J = 64; J = 1; one query past a 256-query workgroup four times over (1025 = 4 * 256 + 1);
# frame boundaries inside a workgroup (171 < 256: the third and later frames of a workgroup read their transforms from global memory); the cfg4 clip
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 100, 1, 24), (3, 5, 70, 257, 64), (1, 2, 300, 2049, 1), (1, 1, 1025, 64, 24), (1, 1, 257, 64, 24), (2, 3, 171, 320, 24),
          (5, 4, 3, 9, 24), (1, 30, 4096, 6890, 24)]


@pytest.mark.parametrize("with_stage1", [False, True])
@pytest.mark.parametrize("clips,T,Vg,V,J", SHAPES)
def test_kernel_against_the_float64_adjoint(clips, T, Vg, V, J, with_stage1):
    F_ = clips * T
    rng = np.random.default_rng(V * 131 + Vg + J)
    idx = dev(rng.integers(0, V, (F_, Vg)).astype(np.int32))
    W, inv_A, A = _weights(F_, V, J, V + 1), _transforms(F_, J, V + 2), _transforms(F_, J, V + 3)
    dp = dev(rng.standard_normal((F_, Vg, 3)).astype(np.float32))
    ds = dev(rng.standard_normal((F_, Vg, 3)).astype(np.float32)) if with_stage1 else None
    got = _grad(clips, T, idx, W, inv_A, A, dp, ds)
    again = _grad(clips, T, idx, W, inv_A, A, dp, ds)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))                       # no atomics: two runs, the same bits
    want, bound = MT.skin_adjoint64(host(idx), host(W), host(inv_A), host(A), host(dp), None if ds is None else host(ds))
    g = host(got).astype(np.float64)
    assert np.isfinite(g).all()
    ratio = np.abs(g - want) / np.maximum(bound, 1e-300)
    print(f"mgn_skin_grad {(clips, T, Vg, V, J)} stage1={with_stage1}: worst err / bound = {ratio.max():.4f} (max |grad| {np.abs(want).max():.3e})")
    assert (np.abs(g - want) <= bound).all(), ratio.max()
    if not with_stage1:   # NULL means zero: the same bits as an explicit zero tensor
        zero = _grad(clips, T, idx, W, inv_A, A, dp, torch.zeros_like(dp))
        assert torch.equal(got.view(torch.int32), zero.view(torch.int32))


def test_adjoint_identity_against_the_forward_kernel():
    """<posed(q + delta) - posed(q), g> from two FORWARD launches equals <delta, grad(g)> from the new kernel: catches a layout misreading shared by
    the kernel and the twin.  The body is a lattice of spacing 0.05, the queries sit within 1e-3 (per coordinate) of a body vertex and move by at
    most 1e-3: no nearest index can change, and every one is checked."""
    clips, T, V, J = 2, 3, 320, 24
    F_ = clips * T
    Vg = 171
    rng = np.random.default_rng(11)
    lattice = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(0.05)
    tpose = np.stack([lattice[rng.permutation(V)] for _ in range(clips)])                                 # (clips,V,3)
    root = (rng.standard_normal((clips, 3)) * 0.01).astype(np.float32)
    u = rng.integers(0, V, (F_, Vg))
    clip = np.arange(F_) // T
    garment = (tpose[clip[:, None], u] + 1e-3 * (rng.random((F_, Vg, 3)) * 2 - 1) - root[clip][:, None, :]).astype(np.float32)
    delta = rng.standard_normal((F_, Vg, 3))
    delta *= (1e-3 * rng.random((F_, Vg, 1))) / np.linalg.norm(delta, axis=-1, keepdims=True)
    garment2 = (garment + delta).astype(np.float32)
    W, inv_A, A = _weights(F_, V, J, 12), _transforms(F_, J, 13), _transforms(F_, J, 14)
    root_d, tpose_d = dev(root), dev(tpose)

    def forward(g):
        idx = torch.empty((F_, Vg), dtype=torch.int32, device="cuda")
        dist = torch.empty((F_, Vg), dtype=torch.float32, device="cuda")
        s1 = torch.empty((F_, Vg, 3), dtype=torch.float32, device="cuda")
        p = torch.empty((F_, Vg, 3), dtype=torch.float32, device="cuda")
        gd = dev(g)
        _lib.call("g4d_mgn_skin_f32", clips, T, Vg, V, J, gd.data_ptr(), root_d.data_ptr(), tpose_d.data_ptr(), W.data_ptr(), inv_A.data_ptr(),
                  A.data_ptr(), idx.data_ptr(), dist.data_ptr(), s1.data_ptr(), p.data_ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()
        return idx, p
    idx1, p1 = forward(garment)
    idx2, p2 = forward(garment2)
    assert np.array_equal(host(idx1), u) and np.array_equal(host(idx2), u)                                # every vertex, none left out
    # g = the sign pattern of the expected difference (float64 twin), so that the terms of <., g> add up instead of cancelling and the identity
    # stands well clear of its tolerance, which is a sum of worst cases
    rootf = root[clip][:, None, :].astype(np.float64)
    g = np.sign(MT.skin64(garment2 + rootf, u, host(W), host(inv_A), host(A))[1] - MT.skin64(garment + rootf, u, host(W), host(inv_A), host(A))[1]).astype(np.float32)
    grad = host(_grad(clips, T, idx1, W, inv_A, A, dev(g))).astype(np.float64)
    lhs = ((host(p2).astype(np.float64) - host(p1).astype(np.float64)) * g).sum()
    rhs = ((garment2.astype(np.float64) - garment.astype(np.float64)) * grad).sum()
    q = garment.astype(np.float64) + root[clip][:, None, :]
    terms = MT.skin64(q, u, host(W), host(inv_A), host(A))[2]
    tol = 2 * (J + 8) * MT.U * (terms * np.abs(g)).sum()
    print(f"adjoint identity: lhs {lhs:.9e} rhs {rhs:.9e} |diff| {abs(lhs - rhs):.3e} tol {tol:.3e}")
    assert abs(lhs) > 20 * tol                                                                            # the identity is not vacuous
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("clips,T,Vg", [(0, 3, 10), (2, 0, 10), (2, 3, 0)])
def test_zero_sizes_launch_nothing(clips, T, Vg):
    sentinel = torch.full((64,), -7.0, device="cuda")
    p = sentinel.data_ptr()
    _lib.call("g4d_mgn_skin_grad_f32", clips, T, Vg, 50, 24, p, p, p, p, p, 0, p, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (sentinel == -7.0).all()


def test_bad_arguments_are_refused():
    F_, Vg, V, J = 2, 8, 16, 8
    idx = torch.zeros((F_, Vg), dtype=torch.int32, device="cuda")
    W, inv_A, A = _weights(F_, V, J, 1), _transforms(F_, J, 2), _transforms(F_, J, 3)
    dp = torch.zeros((F_, Vg, 3), device="cuda")
    out = torch.full((F_, Vg, 3), -7.0, device="cuda")
    ptr = dict(nn_idx=idx.data_ptr(), W=W.data_ptr(), inv_A=inv_A.data_ptr(), A=A.data_ptr(), d_posed=dp.data_ptr(), d_stage1=0, d_garment=out.data_ptr())

    def call(j=J, **kw):
        a = dict(ptr)
        a.update(kw)
        _lib.call("g4d_mgn_skin_grad_f32", 1, F_, Vg, V, j, *a.values(), _lib.stream_ptr())
    for j in (0, 65):
        with pytest.raises(_lib.G4DError, match="1 <= J <= 64"):
            call(j=j)
    for name in ("nn_idx", "W", "inv_A", "A", "d_posed", "d_garment"):
        with pytest.raises(_lib.G4DError, match="null pointer"):
            call(**{name: 0})
    with pytest.raises(_lib.G4DError, match="16-byte aligned"):
        call(A=A.data_ptr() + 4)
    torch.cuda.synchronize()
    assert (out == -7.0).all()


def test_foreign_index_is_clamped():
    """nn_idx holding V and -1 (a stale or foreign index tensor): the kernel clamps before addressing, so such an entry gives the value of vertex V - 1 /
    vertex 0 -- a wrong number, finite, and no read outside W."""
    clips, T, Vg, V, J = 1, 2, 40, 9, 24
    F_ = clips * T
    rng = np.random.default_rng(5)
    good = rng.integers(0, V, (F_, Vg)).astype(np.int32)
    bad = good.copy()
    bad[:, ::3], bad[:, 1::3] = V, -1
    clamped = np.clip(bad, 0, V - 1)
    W, inv_A, A = _weights(F_, V, J, 6), _transforms(F_, J, 7), _transforms(F_, J, 8)
    dp = dev(rng.standard_normal((F_, Vg, 3)).astype(np.float32))
    got = _grad(clips, T, dev(bad), W, inv_A, A, dp)
    assert torch.isfinite(got).all()
    assert torch.equal(got, _grad(clips, T, dev(clamped), W, inv_A, A, dp))


# ---------------------------------------------------------------- lbs_garment_MGN as an autograd node
def _golden_pieces():
    g = MT.load()
    case, targets, sd = MT.golden_inputs()
    assert np.array_equal(g["checksum"], syn.mgn_grad_checksum(case, targets)), "mgn_grad.npz belongs to other inputs: regenerate it"
    return g, case, targets, sd


def _body_model(case):
    body = case["body"]
    return types.SimpleNamespace(parents=torch.from_numpy(body["parents"]).cuda(), faces=body["faces"], J_regressor=dev(body["J_regressor"]),
                                 v_template=dev(body["v_template"]))


def test_skinning_node_same_bits_and_both_outputs_differentiable():
    _, case, _, _ = _golden_pieces()
    b = {k: dev(v) for k, v in case["batch"].items()}
    args = (b["Tpose_smpl_vertices_torch"], b["Tpose_smpl_root_joints_torch"], b["zeropose_smpl_vertices_torch"], _body_model(case).parents, b["pose_torch"],
            b["T_J_regressor"], b["T_lbs_weights"])
    with torch.no_grad():
        posed0, nn0, s0 = lbs_garment_MGN(dev(case["pred_template"]), *args, K=1)
    g = dev(case["pred_template"]).requires_grad_(True)
    posed, nn1, s1 = lbs_garment_MGN(g, *args, K=1)
    assert torch.equal(posed, posed0) and torch.equal(s1, s0) and torch.equal(nn1.idx, nn0.idx) and torch.equal(nn1.dists, nn0.dists)
    assert posed.requires_grad and s1.requires_grad and not nn1.idx.requires_grad and not nn1.dists.requires_grad
    rng = np.random.default_rng(2)
    dp, ds = (dev(rng.standard_normal(tuple(posed.shape)).astype(np.float32)) for _ in range(2))
    ((posed * dp).sum() + (s1 * ds).sum()).backward()
    nbatch, T, Vg = case["nbatch"], case["T"], case["Vg"]
    F_ = nbatch * T
    inv_A, A = MT.transforms64(case["batch"], case["body"]["parents"])
    W = case["batch"]["T_lbs_weights"].reshape(F_, -1, 24)
    want, bound = MT.skin_adjoint64(host(nn0.idx).reshape(F_, Vg), W, inv_A, A, host(dp).reshape(F_, Vg, 3), host(ds).reshape(F_, Vg, 3))
    # the transforms come from the fp32 lbs helpers here and from float64 in the twin: 1e-5 relative on top of the kernel's own bound
    err = np.abs(host(g.grad).reshape(F_, Vg, 3) - want)
    assert (err <= bound + 1e-5 * np.abs(want).max()).all(), err.max()
    only_s1 = dev(case["pred_template"]).requires_grad_(True)
    lbs_garment_MGN(only_s1, *args, K=1)[2].sum().backward()                                  # stage 1 alone: d_posed is zero
    assert torch.isfinite(only_s1.grad).all() and only_s1.grad.abs().max() > 0
    with pytest.raises(NotImplementedError, match="T_lbs_weights"):
        lbs_garment_MGN(g, *args[:-1], b["T_lbs_weights"].clone().requires_grad_(True), K=1)


# ---------------------------------------------------------------- the Linear nodes
def _stack(vg, seed):
    torch.manual_seed(seed)
    seq = torch.nn.Sequential(torch.nn.Linear(512, 1024), torch.nn.ReLU(), torch.nn.Linear(1024, 2048), torch.nn.ReLU(), torch.nn.Linear(2048, 3 * vg)).cuda()
    m = types.SimpleNamespace(displacement_encoder=seq)
    m._displacement_layers = types.MethodType(PCALBSGarmentUseSegEncoderSegMGN._displacement_layers, m)
    return m, [mod for mod in seq if isinstance(mod, torch.nn.Linear)]


@pytest.mark.parametrize("rows", [1, 6, 240])
@pytest.mark.parametrize("vg", [1, 160, 195])
def test_linear_nodes_against_float64_autograd(rows, vg):
    """Each layer's node against torch-float64 autograd of the same layer on the node's own fp32 input and incoming cotangent: the bounds are those
    of the layer's own contractions (rows for dW and db, Cout for dX).  The ReLU decision is the node's (its saved output); where float64 disagrees,
    the pre-activation must lie within the forward's own rounding."""
    holder, mods = _stack(vg, 100 + vg)
    rng = np.random.default_rng(rows * 7 + vg)
    x0 = dev((rng.random((rows, 512)) * rng.random((rows, 512))).astype(np.float32)).requires_grad_(True)
    hs, h = [x0], x0
    for m, layer in zip(mods, holder._displacement_layers()):
        h = _LinearFn.apply(h, m.weight, m.bias, m, layer)
        h.retain_grad()
        hs.append(h)
    dy = dev(rng.standard_normal((rows, 3 * vg)).astype(np.float32))
    h.backward(dy)
    for i, m in enumerate(mods):
        x, y, g_out = host(hs[i]).astype(np.float64), host(hs[i + 1]).astype(np.float64), host(hs[i + 1].grad).astype(np.float64)
        w, b = host(m.weight).astype(np.float64), host(m.bias).astype(np.float64)
        relu = i < 2
        # torch-float64 autograd of the same layer, the ReLU decision held at the node's
        xt, wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, b))
        pre = xt @ wt.t() + bt
        mask = torch.from_numpy((y > 0).astype(np.float64)) if relu else torch.ones_like(pre)
        (pre * mask).backward(torch.from_numpy(g_out))
        if relu:
            fwd_bound = MT.sum_bound(x.shape[1] + 1, np.abs(x) @ np.abs(w).T + np.abs(b))
            differ = (pre.detach().numpy() > 0) != (y > 0)
            assert (np.abs(pre.detach().numpy())[differ] <= fwd_bound[differ]).all()
        (db, b_db), (dw, b_dw), (dx, b_dx) = MT.linear_backward64(x, w, g_out * mask.numpy())
        for mine, auto, bd in ((db, bt.grad, b_db), (dw, wt.grad, b_dw), (dx, xt.grad, b_dx)):   # the twin's formulas ARE torch's float64 autograd
            assert (np.abs(mine - auto.numpy()) <= 1e-4 * bd + 1e-300).all()
        for name, got, want, bound in (("db", m.bias.grad, db, b_db), ("dW", m.weight.grad, dw, b_dw), ("dX", hs[i].grad, dx, b_dx)):
            err = np.abs(host(got).astype(np.float64) - want)
            print(f"linear node rows={rows} vg={vg} layer {i} {name}: worst err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
            assert tuple(got.shape) == want.shape and (err <= bound).all(), (name, i, (err / np.maximum(bound, 1e-300)).max())


def test_relu_outputs_exactly_zero_get_zero_gradient():
    holder, mods = _stack(1, 3)
    with torch.no_grad():
        mods[0].bias[::2] = -100.0                                                            # every second unit of layer 1 is off for every row
    x = dev(np.random.default_rng(0).random((6, 512)).astype(np.float32))
    layer = holder._displacement_layers()[0]
    y = _LinearFn.apply(x, mods[0].weight, mods[0].bias, mods[0], layer)
    assert (y[:, ::2] == 0).all() and (y[:, 1::2] != 0).any()
    y.backward(torch.ones_like(y))
    assert (mods[0].weight.grad[::2] == 0).all() and (mods[0].bias.grad[::2] == 0).all()
    assert (mods[0].bias.grad[1::2] != 0).any() and torch.isfinite(mods[0].weight.grad).all()


# ---------------------------------------------------------------- the model
def _golden_model(case, sd):
    gv = case["template_verts"]
    pca = dict(components=np.zeros((72, gv.size), np.float32), mean=gv.reshape(-1), explained=np.ones(72), ss_scale=np.ones(gv.size))
    m = PCALBSGarmentUseSegEncoderSegMGN(garment_name="Tshirt", pca_dim=64, pca=pca, template=(gv, case["template_faces"]))
    m.displacement_encoder.load_state_dict({k.split(".", 1)[1]: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    enc = dict(tpose_garment=dev(case["tpose_garment"]), garment_summary=dev(case["garment_summary"]))
    m.PCA_garment_encoder.forward = lambda *a, **k: dict(enc)        # the garment encoder's output replaced by the case's, as the generator's stub
    return m


def _golden_call(m, case):
    batch = {k: dev(v) for k, v in case["batch"].items() if k != "smpl_vertices_torch"}
    return m(torch.zeros(case["nbatch"], case["T"], 4, 3, device="cuda"), _body_model(case), batch)


def _loss_inputs(case, targets):
    return dict(pose_torch=dev(case["batch"]["pose_torch"]), **{k: dev(v) for k, v in targets.items()})


def same(a, b, path="out"):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype, path
        if a.is_sparse:
            a, b = a.coalesce(), b.coalesce()
            assert torch.equal(a.indices(), b.indices()) and torch.equal(a.values(), b.values()), path
        else:
            assert torch.equal(a.detach(), b.detach()), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, tuple) and hasattr(a, "_fields"):
        for k in a._fields:
            same(getattr(a, k), getattr(b, k), f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    else:
        assert a is b or a == b, path


def test_forward_under_grad_needs_the_switch():
    """The one test of this file that fails without the feature's model route: with the switch ON the forward runs under grad; OFF it asserts."""
    _, case, _, sd = _golden_pieces()
    m = _golden_model(case, sd)
    with pytest.raises(AssertionError, match="inference only"):
        _golden_call(m, case)
    with on():
        out = _golden_call(m, case)
    assert out["lbs_pred_garment_v"].requires_grad and out["lbs_stage1_pred_garment_v"].requires_grad
    assert len(out["iter_regressed_lbs_garment_v"]) == 1 and out["iter_regressed_lbs_garment_v"][0].requires_grad


def test_forward_under_grad_has_the_inference_bits_golden_case():
    _, case, _, sd = _golden_pieces()
    m = _golden_model(case, sd)
    with torch.no_grad():
        want = _golden_call(m, case)
    with on():
        out = _golden_call(m, case)
        with torch.no_grad():
            again = _golden_call(m, case)                                   # the switch alone changes nothing under no_grad
    same(out, want)
    same(again, want)


def test_forward_under_grad_has_the_inference_bits_195_vertex_scene():
    from garment4d_amd.encoder import seed_encoder
    nbatch, T, N = 2, 3, 2048
    scene = syn.garment_scene(nbatch, T, N, garment_rc=(13, 15), seed=33)
    assert scene["template"][0].shape[0] == 195
    torch.manual_seed(0)
    m = PCALBSGarmentUseSegEncoderSegMGN(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"])
    seed_encoder(m.PCA_garment_encoder, 0)
    m = m.cuda().eval()
    body = scene["body"]
    bm = types.SimpleNamespace(parents=torch.from_numpy(body["parents"]).cuda(), faces=body["faces"], J_regressor=dev(body["J_regressor"]))
    x, batch = dev(scene["x"]), {k: dev(v) for k, v in scene["batch"].items()}
    with torch.no_grad():
        want = m(x, bm, batch)
    with on():
        out = m(x, bm, batch)
        same(out, want)
        out["lbs_pred_garment_v"].square().sum().backward()
        for name, p in m.named_parameters():
            assert (p.grad is None) == name.startswith("PCA_garment_encoder."), name
        with pytest.raises(NotImplementedError, match="bf16"):
            m(x, bm, batch, precision="bf16")
        with pytest.raises(NotImplementedError, match="frame-sharded"):
            m.forward_frames(x.reshape(nbatch * T, N, 3), bm, batch, nbatch=nbatch, T=T, frame_ids=range(nbatch * T))
        next(mod for mod in m.PCA_garment_encoder.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)).train()
        with pytest.raises(AssertionError, match="inference only"):
            m(x, bm, batch)


def test_training_step_matches_the_reference():
    """Model forward + temporal_loss_PCA_LBS + backward() on the golden inputs: every stored gradient and loss scalar within three times the
    reference's own fp32 rounding error (eref) of the reference's fp32 values; no encoder parameter receives a gradient."""
    g, case, targets, sd = _golden_pieces()
    m = _golden_model(case, sd)
    with on():
        out = _golden_call(m, case)
        out["lbs_pred_garment_v"].retain_grad()
        ld = losses.temporal_loss_PCA_LBS(out, _loss_inputs(case, targets), _body_model(case), None, loss_cfg=LOSS_CFG)
        ld["total_loss"].backward()
    failures = []
    for k in ("lbs_garment_msre", "only_lbs_garment_msre", "lbs_garment_l2_loss", "lbs_garment_lap_loss", "lbs_interpenetration_loss",
              "temporal_constraint_loss", "acceleration_error", "only_lbs_acceleration_error", "total_loss"):
        err, eref = abs(float(ld[k]) - float(g[k])), float(g[f"eref_{k}"])
        print(f"training step {k}: |err| {err:.3e}  eref {eref:.3e}  err / (3 eref) {err / (3 * eref):.3f}")
        if err > 3 * eref:
            failures.append((k, err, eref))
    grads = {"displacement_encoder." + n: host(p.grad) for n, p in m.displacement_encoder.named_parameters()}
    F_ = case["nbatch"] * case["T"]
    for k, a in MT.stored_arrays(grads, host(out["lbs_pred_garment_v"].grad).reshape(F_, -1, 3), g).items():
        err, eref = np.abs(a.astype(np.float64) - g[k].astype(np.float64)).max(), float(g[f"eref_{k}"])
        print(f"training step {k}: max |err| {err:.3e}  eref {eref:.3e}  err / (3 eref) {err / (3 * eref):.3f}")
        if err > 3 * eref:
            failures.append((k, err, eref))
    for name, p in m.named_parameters():
        if name.startswith("PCA_garment_encoder."):
            assert p.grad is None, name
    assert not failures, failures


def test_caches_are_rebuilt_after_an_optimizer_step():
    g, case, targets, sd = _golden_pieces()
    m = _golden_model(case, sd)
    opt = torch.optim.Adam(m.displacement_encoder.parameters(), lr=1e-3)
    packs = []
    for _ in range(2):
        with on():
            out = _golden_call(m, case)
            losses.temporal_loss_PCA_LBS(out, _loss_inputs(case, targets), _body_model(case), None, loss_cfg=LOSS_CFG)["total_loss"].backward()
        packs.append([getattr(mod, _cache.ATTR)["packed_t"][1] for mod in m.displacement_encoder if isinstance(mod, torch.nn.Linear) and hasattr(mod, _cache.ATTR)])
        opt.step()
        opt.zero_grad()
    assert len(packs[0]) == 2 and all(a is not b for a, b in zip(*packs))               # layers 2 and 3 only; rebuilt after the step
    fresh = _golden_model(case, {"displacement_encoder." + k: host(v) for k, v in m.displacement_encoder.state_dict().items()})
    with torch.no_grad():
        same(_golden_call(m, case), _golden_call(fresh, case))
    with on():
        a, b = _golden_call(m, case), _golden_call(fresh, case)
        same(a, b)
        for mm, o in ((m, a), (fresh, b)):
            mm.zero_grad()
            o["lbs_pred_garment_v"].square().sum().backward()
    for p, q in zip(m.displacement_encoder.parameters(), fresh.displacement_encoder.parameters()):
        assert torch.equal(p.grad, q.grad)                                               # the transposed packs too


def test_ten_adam_steps_lower_the_loss():
    """Ten Adam steps at lr 1e-3 on the golden batch (tests/test_mgn_grad_cpu.py shows the float64 twin of the reference computation decreasing on
    it, seed 90 / target seed 190, the first tried)."""
    g, case, targets, sd = _golden_pieces()
    m = _golden_model(case, sd)
    opt = torch.optim.Adam(m.displacement_encoder.parameters(), lr=1e-3)
    inputs, bm = _loss_inputs(case, targets), _body_model(case)
    history = []
    with on():
        for step in range(11):
            ld = losses.temporal_loss_PCA_LBS(_golden_call(m, case), inputs, bm, None, loss_cfg=LOSS_CFG)
            history.append(float(ld["total_loss"]))
            if step < 10:
                opt.zero_grad()
                ld["total_loss"].backward()
                opt.step()
    print("total_loss over ten Adam steps:", " ".join(f"{v:.5f}" for v in history))
    assert history[10] < history[0]


def test_nan_row_in_the_last_weight():
    """A NaN row of displacement_encoder.4.weight: the forward writes 0 at its coordinate, the cotangent there is exactly 0, every other gradient
    stays finite (the row's own gradient is G^T X with G = 0 there: zero, not NaN)."""
    _, case, _, sd = _golden_pieces()
    m = _golden_model(case, sd)
    rows = torch.tensor([0, 7, 100], device="cuda")
    with torch.no_grad():
        m.displacement_encoder[4].weight[rows] = float("nan")
    summary = dev(case["garment_summary"]).reshape(-1, 512)
    with on():
        d = m.displacements(summary)
        flat = d.reshape(d.shape[0], -1)
        assert (flat[:, rows] == 0).all() and torch.isfinite(d).all()
        seen = []
        h = d.grad_fn.next_functions[0][0]                       # the node of `* 0.05`: what reaches it is the displacement cotangent after the mask
        h.register_hook(lambda grad_in, grad_out: seen.append(grad_out[0]))
        d.sum().backward()
    cot = seen[0].reshape(seen[0].shape[0], -1)
    assert (cot[:, rows] == 0).all() and (cot != 0).any()
    last = m.displacement_encoder[4]
    assert (last.bias.grad[rows] == 0).all() and (last.weight.grad[rows] == 0).all()
    keep = torch.ones(last.bias.numel(), dtype=torch.bool, device="cuda")
    keep[rows] = False
    assert (last.bias.grad[keep] != 0).all()
    for p in m.displacement_encoder.parameters():
        assert torch.isfinite(p.grad).all()
