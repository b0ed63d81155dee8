"""Time one MGN training iteration (train_temporal.py --MGN 1) at the cfg4 shape (8 clips x 30 frames, Vg = 4096, V = 6890, J = 24) on one GPU:
  (a) the trained part, forward + backward: displacement MLP (mesh_encoder._LinearFn on g4d_linear_f32 / g4d_gemm_tn_f32 / g4d_col_sum_rows_f32),
        * 0.05 / NaN guard, skinning (garment_lbs._MGNSkinFn: g4d_mgn_skin_f32 forward INCLUDING its nearest-vertex search, g4d_mgn_skin_grad_f32
        backward) and the objective (losses.stage2_loss, one round); the joint transforms are given.
  (b) the same computation as torch ops + torch's autograd on the same GPU: nn.Sequential, the reference's matmul / gather blends
        (modules/mesh_encoder.py:553-583) GIVEN the nearest index and the transforms, the objective as the reference writes it
        (smplx/loss/temporal_loss.py).  The BASELINE, not the code under test.  It does not pay for the skinning's search; (a) does
        (`skin_forward_ms` is that launch alone).  Both take the loss's nearest body vertex from fused.three_nn inside the timed region.
  (c) a whole step: PCALBSGarmentUseSegEncoderSegMGN.forward under grad (tuning.Tuning.mgn_autograd: encoder under no_grad), temporal_loss_PCA_LBS,
        total_loss.backward(), torch.optim.Adam.step() over the six displacement_encoder parameters.
  (d) launches alone: g4d_mgn_skin_grad_f32, and each of the three weight-gradient g4d_gemm_tn_f32 launches (240 rows; torch's G^T X next to each).
Protocol of scripts/time_stage2_step.py: device events around each call after a warm-up; median and minimum.  One JSON line.
usage: python scripts/time_mgn_step.py [clips] [T] [side] [iters] [step: 0|1]      (Vg = side x side)"""
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from garment4d_amd import fused, grad_ops, losses, tuning
from garment4d_amd import lbs as L
from garment4d_amd import synthetic as syn
from garment4d_amd.garment_lbs import _MGNSkinFn, _mgn_skin
from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSegMGN, _packed_transposed

clips = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 30
side = int(sys.argv[3]) if len(sys.argv) > 3 else 64
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 7
with_step = (int(sys.argv[5]) if len(sys.argv) > 5 else 1) != 0
assert torch.cuda.is_available(), "time_mgn_step.py measures on the GPU"
F_, Vg, N, J = clips * T, side * side, 8192, 24
LAMBDAS = (20.0, 10.0, 100.0, 5.0)            # cfgs/tshirt.yaml
LOSS_CFG = dict(zip(losses.LOSS_LAMBDAS, LAMBDAS))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def timed(fn, n=iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


rng = np.random.default_rng(0)
scene = syn.garment_scene(clips, T, N if with_step else 4, body_rc=(65, 106), garment_rc=(side, side), seed=1)
body = scene["body"]
b = {k: dev(v) for k, v in scene["batch"].items()}
V = body["v_template"].shape[0]
parents = torch.from_numpy(body["parents"]).cuda()
bm = types.SimpleNamespace(parents=parents, faces=body["faces"], J_regressor=dev(body["J_regressor"]), v_template=dev(body["v_template"]))
torch.manual_seed(0)
m = PCALBSGarmentUseSegEncoderSegMGN(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"])
if with_step:
    from garment4d_amd.encoder import seed_encoder
    seed_encoder(m.PCA_garment_encoder, 0)
m = m.cuda().eval()
on = tuning.current().replace(mgn_autograd=True)

# the constants of the trained part: garment summary, PCA garment, transforms, loss operands
summary = dev((rng.random((F_, 512)) * rng.random((F_, 512))).astype(np.float32))
tpose_garment = dev((scene["template"][0][None] + rng.standard_normal((clips, Vg, 3)) * 0.004).astype(np.float32))
with torch.no_grad():
    Jreg = b["T_J_regressor"].reshape(F_, J, V).contiguous()
    tbody = b["Tpose_smpl_vertices_torch"].reshape(clips, V, 3).contiguous()
    tbody_f = tbody.reshape(clips, 1, V, 3).expand(clips, T, V, 3).reshape(F_, V, 3).contiguous()
    inv_pose = torch.zeros((F_, 24, 3), device="cuda")
    inv_pose[:, 0, 0], inv_pose[:, 1, 1], inv_pose[:, 2, 1] = -np.pi / 2, 0.15, -0.15
    _, inv_A = L.batch_rigid_transform(L.batch_rodrigues(inv_pose.reshape(-1, 3)).reshape(F_, 24, 3, 3), L.vertices2jointsB(Jreg, tbody_f), parents)
    _, A = L.batch_rigid_transform(L.batch_rodrigues(b["pose_torch"].reshape(-1, 3)).reshape(F_, 24, 3, 3),
                                   L.vertices2jointsB(Jreg, b["zeropose_smpl_vertices_torch"].reshape(F_, V, 3).contiguous()), parents)
    W = b["T_lbs_weights"].reshape(F_, V, J).contiguous()
    root = b["Tpose_smpl_root_joints_torch"].reshape(clips, 3).contiguous()
    body_v = b["smpl_vertices_torch"].reshape(F_, V, 3).contiguous()
    body_vn = dev(syn.vertex_normals(scene["batch"]["smpl_vertices_torch"].reshape(F_, V, 3), body["faces"]))
    lap_adj = m._lap_adj_on(torch.device("cuda")).coalesce()
    with tuning.use(on):
        d0 = m.displacements(summary)
    idx0, _, _, posed0 = _mgn_skin(clips, T, (tpose_garment[:, None] + d0.reshape(clips, T, Vg, 3)).reshape(F_, Vg, 3).contiguous(), root, tbody, W, inv_A, A)
    target = (posed0 + torch.randn_like(posed0) * 0.01).contiguous()
    idx_long = idx0.long()
params = list(m.displacement_encoder.parameters())
seq = m.displacement_encoder


def hip_part():
    with tuning.use(on):
        d = m.displacements(summary)
    garment = (tpose_garment[:, None] + d.reshape(clips, T, Vg, 3)).reshape(F_, Vg, 3).contiguous()
    posed = _MGNSkinFn.apply(garment, root, tbody, W, inv_A, A, clips, T)[0]
    total = losses.stage2_loss([posed], target, body_v, body_vn, lap_adj, clips, T, LAMBDAS)[0]
    return total, torch.autograd.grad(total, params)


def torch_part():
    d = seq(summary).reshape(F_, Vg, 3) * 0.05
    d = d.masked_fill(torch.isnan(d), 0.0)
    q = (tpose_garment[:, None] + d.reshape(clips, T, Vg, 3) + root.reshape(clips, 1, 1, 3)).reshape(F_, Vg, 3)
    rep = idx_long.reshape(F_, -1, 1, 1).repeat(1, 1, 4, 4)
    ones = torch.ones((F_, Vg, 1), device="cuda")
    inv_nn_T = torch.gather(torch.matmul(W, inv_A.view(F_, J, 16)).view(F_, V, 4, 4), 1, rep)
    s = torch.matmul(inv_nn_T, torch.cat([q, ones], 2).unsqueeze(-1))[:, :, :3, 0]
    nn_T = torch.gather(torch.matmul(W, A.view(F_, J, 16)).view(F_, V, 4, 4), 1, rep)
    p = torch.matmul(nn_T, torch.cat([s, ones], 2).unsqueeze(-1))[:, :, :3, 0]
    l2 = ((p - target) ** 2).sum(-1).mean()
    msre = torch.sqrt(((p - target) ** 2).sum(-1)).mean(-1)      # the metric the reference computes on the way
    pl = torch.spmm(lap_adj, p.transpose(0, 1).reshape(-1, F_ * 3)).reshape(-1, F_, 3).transpose(0, 1)
    lap = torch.norm(pl, p=2, dim=-1).mean()
    with torch.no_grad():
        idx = fused.three_nn(p.detach().contiguous(), body_v)[1][..., :1].long()
    ex = idx.expand(idx.size(0), idx.size(1), 3)
    pen = torch.relu(-torch.mul(torch.gather(body_vn, 1, ex), p - torch.gather(body_v, 1, ex)).sum(-1)).mean()
    last = p.reshape(clips, T, -1, 3)
    tmp = ((last[:, :-1] - last[:, 1:]) ** 2).sum(-1).sqrt().mean()
    total = l2 * LAMBDAS[0] + lap * LAMBDAS[1] + pen * LAMBDAS[2] + tmp * LAMBDAS[3]
    return total, torch.autograd.grad(total, params), msre


out = dict(shape=dict(clips=clips, T=T, frames=F_, Vg=Vg, body=V, J=J))
a, c = hip_part(), torch_part()
out["total_hip"], out["total_torch"] = float(a[0].detach()), float(c[0].detach())
out["grad_max_abs_diff"] = [float((x - y).abs().max()) for x, y in zip(a[1], c[1])]
out["grad_max_abs"] = [float(y.abs().max()) for y in c[1]]
del a, c
out["part_hip_ms"], out["part_hip_min_ms"] = timed(hip_part)
out["part_torch_ms"], out["part_torch_min_ms"] = timed(torch_part)
out["part_speedup"] = out["part_torch_ms"] / out["part_hip_ms"]
torch.cuda.empty_cache()

# ---- (d) launches alone
with torch.no_grad():
    gq = (tpose_garment[:, None] + d0.reshape(clips, T, Vg, 3)).reshape(F_, Vg, 3).contiguous()
    out["skin_forward_ms"] = timed(lambda: _mgn_skin(clips, T, gq, root, tbody, W, inv_A, A))[0]
    dp = torch.randn(F_, Vg, 3, device="cuda")
    out["skin_grad_ms"], out["skin_grad_min_ms"] = timed(lambda: grad_ops.mgn_skin_grad(clips, T, idx0, W, inv_A, A, dp))
    out["skin_grad_GB_per_s"] = (F_ * Vg * (3 * 4 * 2 + 4 + J * 4)) / (out["skin_grad_ms"] * 1e-3) / 1e9     # cotangent in, gradient out, index, W row
    for cin, cout in ((512, 1024), (1024, 2048), (2048, 3 * Vg)):
        G, X = torch.randn(F_, cout, device="cuda"), torch.randn(F_, cin, device="cuda")
        key = f"dW_{cout}x{cin}"
        out[key + "_gemm_tn_ms"] = timed(lambda: grad_ops.gemm_tn(F_, cout, cout, cin, G, X))[0]
        out[key + "_torch_ms"] = timed(lambda: G.t() @ X)[0]
        Wt = torch.randn(cout, cin, device="cuda")
        lin = torch.nn.Linear(cin, cout).cuda()
        out[f"dX_{cout}to{cin}_linear_ms"] = timed(lambda: fused.linear(G, _packed_transposed(lin)))[0]
        out[f"dX_{cout}to{cin}_torch_ms"] = timed(lambda: G @ Wt)[0]
        del G, X, Wt, lin
torch.cuda.empty_cache()

# ---- (c) a whole step
if with_step:
    x = dev(scene["x"])
    with torch.no_grad():
        posed = m(x, bm, b)["lbs_pred_garment_v"]
    rootj = dev(rng.normal(0.0, 0.05, (clips, T, 3)).astype(np.float32))
    inputs = dict(pose_torch=b["pose_torch"], smpl_vertices_torch=b["smpl_vertices_torch"], smpl_root_joints_torch=rootj,
                  garment_torch=posed.reshape(clips, T, Vg, 3) + torch.randn(clips, T, Vg, 3, device="cuda") * 0.01 - rootj[:, :, None, :])
    opt = torch.optim.Adam(params, lr=1e-5)

    def forward_only():
        with torch.no_grad():
            return m(x, bm, b)

    def step():
        opt.zero_grad(set_to_none=True)
        with tuning.use(on):
            od = m(x, bm, b)
        ld = losses.temporal_loss_PCA_LBS(od, inputs, bm, None, loss_cfg=LOSS_CFG)
        ld["total_loss"].backward()
        opt.step()
        return ld["total_loss"]

    first = float(step().detach())
    out["step_ms"], out["step_min_ms"] = timed(step, n=max(3, iters // 2), warm=1)
    out["step_total_loss_first_last"] = [first, float(step().detach())]
    out["inference_forward_ms"] = timed(forward_only, n=max(3, iters // 2), warm=1)[0]
    out["step_frames_per_s"] = F_ / (out["step_ms"] * 1e-3)
print(json.dumps(out))
