"""The stage-2 objective on the GPU (garment4d_amd/csrc/refine_loss.hip, losses.temporal_loss_PCA_LBS, the model class under grad).

Kernel against the float64 twin of tests/stage2_loss_twin.py, value by value and gradient element by gradient element, within the bounds the
twin derives from the kernel's documented arithmetic and reduction tree (nothing in them is a measured number).  Vertices where two correct
fp32 evaluations may take different decisions (penetration sign, nearest body vertex, a near-zero Laplacian or frame difference) are flagged by
the twin alone and left out of the gradient comparison on both sides; the flagged share must stay below 1 % in every case (asserted: the inputs
change if it does not, never the cap).  The reference's own run (tests/golden/stage2_loss.npz): per gradient tensor
max |hip - ref64| <= 3 e_ref, e_ref = max |ref32 - ref64| (the rule of gcn_grad.npz and refine_grad.npz); per scalar the larger of 3 e_ref and
the twin's bound for OUR reduction tree, whose order differs from torch's."""
import types

import numpy as np
import pytest
import torch

import stage2_loss_twin as TW
from garment4d_amd import fused, losses, synthetic as syn, tuning
from garment4d_amd.encoder import seed_encoder
from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSeg, label_dict

pytestmark = pytest.mark.gpu
U = TW.U
ALL = TW.LAMBDAS
WEIGHTS = {"l2": (ALL[0], 0.0, 0.0, 0.0), "lap": (0.0, ALL[1], 0.0, 0.0), "pen": (0.0, 0.0, ALL[2], 0.0), "tmp": (0.0, 0.0, 0.0, ALL[3]), "all": ALL}
LOSS_CFG = dict(zip(losses.LOSS_LAMBDAS, ALL))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def hip_round(c, weights, grad=True):
    """One round through losses.stage2_loss.  Returns (total, vals (5,), msre_frames, grad or None) as numpy / float."""
    p = dev(c["p"]).requires_grad_(grad)
    total, vals, msre = losses.stage2_loss([p], dev(c["g"]), dev(c["body"]), dev(c["normals"]), c["L"], c["nbatch"], c["T"], weights)
    g = None
    if grad:
        total.backward()
        g = host(p.grad)
    torch.cuda.synchronize()
    return float(total.detach()), host(vals)[0], host(msre), g


# Vg = 64, ragged 195 (13 x 15), 4096 -- and 16384 (128 x 128), whose p alone (192 KB) is beyond the 160 KB of LDS a workgroup has: the kernel
# stages u through global memory for every size, so this is the same route; T = 1 has no temporal term
CASES = [(8, 8, 2, 1), (8, 8, 2, 3), (8, 8, 2, 30), (13, 15, 2, 1), (13, 15, 2, 3), (13, 15, 1, 30), (64, 64, 1, 1), (64, 64, 1, 3), (64, 64, 1, 30),
         (128, 128, 1, 3)]


@pytest.mark.parametrize("rows,cols,nbatch,T", CASES)
def test_kernel_against_the_twin(rows, cols, nbatch, T):
    c = TW.garment_case(100 + rows + T, nbatch, T, rows, cols)
    F_, Vg = nbatch * T, rows * cols
    r = TW.evaluate(c["p"], c["g"], c["body"], c["normals"], c["L"], nbatch, T)
    fl = TW.flags(r)
    share = fl.mean()
    print(f"Vg {Vg} F {F_}: flagged {share:.5f}, penetrating {(r['dot'] < 0).mean():.3f}, reduction depth {TW.reduction_depth(F_, Vg)}")
    assert share <= 0.01, share
    assert 0.2 <= (r["dot"] < 0).mean() <= 0.8
    idx = host(fused.three_nn(dev(c["p"]), dev(c["body"]))[1][..., 0])
    assert np.array_equal(idx[~fl], r["idx"][~fl]), "nearest body vertex differs outside the flagged set"
    for name, w in WEIGHTS.items():
        total, vals, msre, g = hip_round(c, w)
        for k, term in enumerate(TW.TERMS):                       # a term with weight 0 is still reported
            err, bound = abs(float(vals[k]) - r["values"][term]), r["value_bounds"][term]
            print(f"  [{name}] {term}: {float(vals[k]):.9g} twin {r['values'][term]:.9g} err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (name, term, err, bound)
        if T == 1:
            assert vals[4] == 0.0
        assert (np.abs(msre - r["msre_frames"]) <= r["msre_frames_bound"]).all()
        want_total = TW.total([r["values"]], w)
        assert abs(total - want_total) <= TW.total_bound([r["values"]], [r["value_bounds"]], w), (name, total, want_total)
        want, bound = TW.gradient(r, w)
        assert np.isfinite(g).all()
        err = np.abs(g - want)
        keep = ~fl
        worst = (err[keep] / np.maximum(bound[keep], 1e-300)).max()
        print(f"  [{name}] gradient: max |g| {np.abs(want).max():.3e}, max err {err[keep].max():.3e}, worst err / bound {worst:.3f}")
        assert (err[keep] <= bound[keep]).all(), (name, float(worst))
        if name != "all":                                        # one term alone: where the twin's gradient is exactly zero, so is the kernel's
            assert (g[keep][want[keep] == 0.0] == 0.0).all()


def golden_setup():
    g, case = TW.load(), syn.stage2_loss_case()
    assert np.array_equal(g["checksum"], syn.stage2_loss_checksum(case)), "stage2_loss.npz belongs to other inputs: regenerate it"
    body = case["body"]
    bm = types.SimpleNamespace(faces=body["faces"], v_template=dev(body["v_template"]))
    lap = G_lap(case["template_faces"], case["Vg"])
    inputs = {k: dev(v) for k, v in case["inputs"].items()}
    return g, case, bm, lap, inputs


def G_lap(faces, vg):
    from garment4d_amd import gcn
    return gcn.sparse_mx_to_torch_sparse_tensor(TW.laplacian_from_faces(faces, vg)).cuda()


def test_golden_reference_run():
    g, case, bm, lap, inputs = golden_setup()
    rounds = [dev(p).requires_grad_(True) for p in case["rounds"]]
    od = dict(iter_regressed_lbs_garment_v=rounds, lbs_pred_garment_v=dev(case["lbs_pred_garment_v"]), lap_adj=lap)
    ld = losses.temporal_loss_PCA_LBS(od, inputs, bm, None, loss_cfg=LOSS_CFG)
    assert set(ld) == {"lbs_garment_msre", "lbs_garment_msre_list", "only_lbs_garment_msre", "lbs_garment_l2_loss", "lbs_garment_lap_loss",
                       "lbs_interpenetration_loss", "temporal_constraint_loss", "acceleration_error", "only_lbs_acceleration_error", "total_loss"}
    ld["total_loss"].backward()
    # ref64 = the twin, which tests/test_stage2_loss_cpu.py ties to the stored float64 figures; its float64 normals differ from the product's
    # fp32 ones (g4d_vertex_normals_f32) by 22 roundings per component -- edge differences 1, cross product 3, face norm + division 5, up to
    # 8 incident faces 8, vertex norm + division 5 -- times the cross product's cancellation factor 1 / sin(angle) <= 2 on this body's
    # right-angled triangles, and one more for good measure: 64 u, carried into the penetration term's bound
    p_rounds, gt, body, normals, L, nbatch, T = TW.golden_inputs(case)
    F_, Vg = nbatch * T, case["Vg"]
    rs = [TW.evaluate(p, gt, body, normals, L, nbatch, T, temporal=(i == 2)) for i, p in enumerate(p_rounds)]
    vals, bounds = [r["values"] for r in rs], [dict(r["value_bounds"]) for r in rs]
    for r, b in zip(rs, bounds):
        b["pen"] += (64 * U * np.abs(np.asarray(r["p_minus_b"])).sum(-1)).sum() / (F_ * Vg)
    n = F_ * Vg
    lbs_pred = case["lbs_pred_garment_v"].reshape(F_, Vg, 3).astype(np.float64)
    ms_lbs = np.sqrt(((lbs_pred - gt) ** 2).sum(-1))
    ref = {
        "lbs_garment_msre": (vals[-1]["msre"], bounds[-1]["msre"]),
        "lbs_garment_l2_loss": (sum(v["l2"] for v in vals), sum(b["l2"] for b in bounds) + 3 * U * sum(v["l2"] for v in vals)),
        "lbs_garment_lap_loss": (sum(v["lap"] for v in vals), sum(b["lap"] for b in bounds) + 3 * U * sum(v["lap"] for v in vals)),
        "lbs_interpenetration_loss": (sum(v["pen"] for v in vals), sum(b["pen"] for b in bounds) + 3 * U * sum(v["pen"] for v in vals)),
        "temporal_constraint_loss": (vals[-1]["tmp"], bounds[-1]["tmp"]),
        "total_loss": (TW.total(vals, ALL), TW.total_bound(vals, bounds, ALL)),
        # plain torch reductions, whose order is torch's: any order of n terms errs by at most (n - 1) u sum |x|
        "only_lbs_garment_msre": (ms_lbs.mean(), (4 + n) * U * ms_lbs.mean()),
        "acceleration_error": (TW.acceleration_error(p_rounds[-1], gt, nbatch, T), TW.acceleration_error_bound(p_rounds[-1], gt, nbatch, T)),
        "only_lbs_acceleration_error": (TW.acceleration_error(lbs_pred, gt, nbatch, T), TW.acceleration_error_bound(lbs_pred, gt, nbatch, T)),
    }
    for k, (want, bound) in ref.items():
        assert abs(want - float(g[f"f64_{k}"])) <= 1e-11 * max(abs(want), 1e-3), k
        err, allowed = abs(float(ld[k].detach()) - want), max(3 * float(g[f"eref_{k}"]), bound)
        print(f"{k}: {float(ld[k].detach()):.9g} ref64 {want:.9g} err {err:.3e}; 3 e_ref {3 * float(g['eref_' + k]):.3e}, bound {bound:.3e}")
        assert err <= allowed, (k, err, allowed)
    assert ld["lbs_garment_msre_list"].shape == (nbatch, T)
    assert (np.abs(host(ld["lbs_garment_msre_list"]).reshape(-1) - rs[-1]["msre_frames"]) <= rs[-1]["msre_frames_bound"]).all()
    ratios = {}
    for i, r in enumerate(rs):
        want, _ = TW.gradient(r, ALL if i == 2 else ALL[:3] + (0.0,))
        e = float(np.abs(host(rounds[i].grad).astype(np.float64) - want).max())
        ratios[i] = e / float(g[f"eref_grad{i}"])
        print(f"grad{i}: max |hip - ref64| = {e:.3e}, e_ref = {float(g[f'eref_grad{i}']):.3e}, ratio {ratios[i]:.2f}")
    bad = {k: round(v, 2) for k, v in ratios.items() if v > 3.0}
    assert not bad, f"beyond 3 e_ref: {bad}"


def test_bit_reproducible():
    c = TW.garment_case(7, 1, 3, 64, 64)
    a, b = hip_round(c, ALL), hip_round(c, ALL)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_no_grad_route_has_the_same_bits():
    g, case, bm, lap, inputs = golden_setup()
    od = dict(iter_regressed_lbs_garment_v=[dev(p).requires_grad_(True) for p in case["rounds"]], lbs_pred_garment_v=dev(case["lbs_pred_garment_v"]),
              lap_adj=lap)
    with_grad = losses.temporal_loss_PCA_LBS(od, inputs, bm, None, loss_cfg=LOSS_CFG)
    assert with_grad["total_loss"].requires_grad
    with torch.no_grad():
        without = losses.temporal_loss_PCA_LBS(od, inputs, bm, None, loss_cfg=LOSS_CFG)
    od2 = dict(od, iter_regressed_lbs_garment_v=[p.detach() for p in od["iter_regressed_lbs_garment_v"]])
    leafless = losses.temporal_loss_PCA_LBS(od2, inputs, bm, None, loss_cfg=LOSS_CFG)       # grad enabled, but nothing requires it
    for other in (without, leafless):
        assert not other["total_loss"].requires_grad and other["total_loss"].grad_fn is None
        for k in with_grad:
            assert torch.equal(with_grad[k].detach(), other[k]), k
    # one round's penetration term against calc_interpenetration_loss: the per-vertex penalties are the same bits, the reductions differ
    # (ours: the documented tree; torch's mean: any order, at most (n - 1) u sum |x|)
    nbatch, T, Vg = case["nbatch"], case["T"], case["Vg"]
    F_ = nbatch * T
    so = {"vertices": inputs["smpl_vertices_torch"].reshape(F_, -1, 3), "joints": inputs["smpl_root_joints_torch"].reshape(F_, 1, 3)}
    p0 = dev(case["rounds"][0])
    want = float(losses.calc_interpenetration_loss(bm, so, p0, reduce_fn="mean"))
    one = losses.temporal_loss_PCA_LBS(dict(od, iter_regressed_lbs_garment_v=[p0]), inputs, bm, None, loss_cfg=LOSS_CFG)
    got = float(one["lbs_interpenetration_loss"])
    assert abs(got - want) <= (TW.reduction_depth(F_, Vg) + 2 + F_ * Vg) * U * abs(want), (got, want)


def flat_patch(n):
    """An n x n open quad grid in the plane z = 0 with spacing 1/8: every interior vertex has four neighbours placed symmetrically, so its
    (L p) is exactly zero in any arithmetic."""
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    verts = np.stack([ii * 0.125, jj * 0.125, np.zeros_like(ii, dtype=np.float64)], -1).reshape(-1, 3).astype(np.float32)
    faces = [[i * n + j, i * n + j + 1, (i + 1) * n + j + 1, (i + 1) * n + j] for i in range(n - 1) for j in range(n - 1)]
    return verts, np.asarray(faces, dtype=np.int32)


def test_zero_norms_contribute_nothing():
    n, nbatch, T = 12, 1, 3
    verts, faces = flat_patch(n)
    Vg, F_ = n * n, nbatch * T
    L = TW.laplacian_from_faces(faces, Vg)
    p = np.repeat(verts[None], F_, 0).copy()
    p[2, :, 0] += np.float32(0.25)                              # frames 0 and 1 identical, frame 2 translated (L p unchanged)
    rng = np.random.default_rng(3)
    body = rng.standard_normal((F_, 50, 3)).astype(np.float32)
    normals = body / np.linalg.norm(body, axis=-1, keepdims=True)
    c = dict(p=p, g=p + np.float32(0.5), body=body, normals=normals.astype(np.float32), L=L, nbatch=nbatch, T=T)
    interior = np.zeros((n, n), bool)
    interior[2:-2, 2:-2] = True                                # its whole row of L^T is interior: no boundary vertex reaches it
    interior = interior.reshape(-1)
    _, vals, _, g = hip_round(c, WEIGHTS["lap"])
    assert np.isfinite(vals).all() and np.isfinite(g).all()
    assert (g[:, interior] == 0.0).all() and np.abs(g).max() > 0       # zero (L p) -> zero contribution; the boundary still has a gradient
    _, vals, _, g = hip_round(c, WEIGHTS["tmp"])
    assert np.isfinite(vals).all() and np.isfinite(g).all()            # the reference's sqrt gives NaN here (inf * 0): DESIGN.md section 8
    assert (g[0] == 0.0).all()                                         # frame 0's only pair has zero length
    assert (g[1] != 0.0).any() and np.allclose(g[1], -g[2])            # the pair (1, 2) pulls both frames
    assert vals[4] == pytest.approx(0.25 / 2, rel=1e-6)                # mean over the two pairs: 0 and 0.25


def test_a_target_that_requires_grad_is_refused():
    c = TW.garment_case(9, 1, 3, 8, 8)
    p = dev(c["p"]).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="target"):
        losses.stage2_loss([p], dev(c["g"]).requires_grad_(True), dev(c["body"]), dev(c["normals"]), c["L"], 1, 3, ALL)
    with pytest.raises(NotImplementedError, match="body_vn"):
        losses.stage2_loss([p], dev(c["g"]), dev(c["body"]), dev(c["normals"]).requires_grad_(True), c["L"], 1, 3, ALL)


# ---- the model class -------------------------------------------------------------------------------------------------------------------------
def small_model(scene, seed=0):
    """tests/test_model_gpu.py's small model: seeded encoder, the head's constructor initialisation halved, ~35 % garment points."""
    torch.manual_seed(seed)
    m = PCALBSGarmentUseSegEncoderSeg(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"], lbs_k=16, iteration=3)
    seed_encoder(m.PCA_garment_encoder, seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if not name.startswith("PCA_garment_encoder."):
                p.mul_(0.5)
    m = m.cuda().eval()
    with torch.no_grad():
        x = dev(scene["x"]).reshape(-1, scene["x"].shape[2], 3)
        logits = m.PCA_garment_encoder.pointnet.forward_fused(x)[1]
        tgt = label_dict["Tshirt"] - 1
        others = torch.cat([logits[..., :tgt], logits[..., tgt + 1:]], -1).max(-1)[0]
        m.PCA_garment_encoder.pointnet.FC_layer[2].conv.bias[tgt] += torch.quantile((others - logits[..., tgt]).flatten(), 0.35)
    return m


def same(a, b, path="out"):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape, path
        if a.is_sparse:
            a, b = a.to_dense(), b.to_dense()
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


def test_model_class_trains_the_head_only():
    """The small model of tests/test_model_gpu.py on the body and the 64-vertex template of refine_golden_case (an 8 x 8 garment cylinder) with a
    real point cloud -- refine_golden_case itself carries four points per frame, which no encoder can run on."""
    nbatch, T, N = 2, 3, 2048
    scene = syn.garment_scene(nbatch, T, N, garment_rc=(8, 8), seed=70)
    m = small_model(scene)
    body = scene["body"]
    bm = types.SimpleNamespace(parents=torch.from_numpy(body["parents"]).cuda(), faces=body["faces"], J_regressor=dev(body["J_regressor"]),
                               v_template=dev(body["v_template"]))
    x, batch = dev(scene["x"]), {k: dev(v) for k, v in scene["batch"].items()}
    with torch.no_grad():
        want = m(x, bm, batch)
    with pytest.raises(AssertionError, match="inference only"):           # the switch off: as it always was
        m(x, bm, batch)
    on = tuning.current().replace(refine_autograd=True)
    m.train()                                                              # the head's modules may be in either mode ...
    m.PCA_garment_encoder.eval()                                           # ... the encoder must be entirely in eval()
    with tuning.use(on):
        out = m(x, bm, batch)
    assert set(out) == set(want)
    same(out, want)
    assert all(o.requires_grad for o in out["iter_regressed_lbs_garment_v"]) and not out["lbs_pred_garment_v"].requires_grad
    rng = np.random.default_rng(71)
    Vg = out["lbs_pred_garment_v"].shape[-2]
    root = rng.normal(0.0, 0.05, (nbatch, T, 3)).astype(np.float32)
    garment = host(out["lbs_pred_garment_v"]).reshape(nbatch, T, Vg, 3) + rng.normal(0.0, 0.01, (nbatch, T, Vg, 3)).astype(np.float32) - root[:, :, None]
    inputs = dict(pose_torch=batch["pose_torch"], smpl_vertices_torch=batch["smpl_vertices_torch"], smpl_root_joints_torch=dev(root),
                  garment_torch=dev(garment.astype(np.float32)))
    opt = torch.optim.Adam([p for n, p in m.named_parameters() if not n.startswith("PCA_garment_encoder.")], lr=1e-4)
    ld = losses.temporal_loss_PCA_LBS(out, inputs, bm, None, loss_cfg=LOSS_CFG)
    assert torch.isfinite(ld["total_loss"]) and ld["total_loss"].requires_grad
    ld["total_loss"].backward()
    for name, p in m.named_parameters():
        if name.startswith("PCA_garment_encoder."):
            assert p.grad is None, name
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.step()
    moved = [n for n, p in m.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert moved and not [n for n in moved if n.startswith("PCA_garment_encoder.")]
    with tuning.use(on):                                                   # a BatchNorm of the encoder back in train(): refused
        next(mod for mod in m.PCA_garment_encoder.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)).train()
        with pytest.raises(AssertionError, match="inference only"):
            m(x, bm, batch)
