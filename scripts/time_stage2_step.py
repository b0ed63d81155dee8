"""Time one stage-2 training iteration at the cfg4 shape (8 clips x 30 frames, 4096 garment / 6890 body vertices, three rounds) on one GPU:
  (a) the objective alone, forward + backward w.r.t. the three round outputs:
        hip     losses.stage2_loss: one g4d_refine_loss_f32 call per round (csrc/refine_loss.hip) + the nearest-vertex search
        torch   the same objective as plain torch ops + torch's autograd on the same GPU, in the reference's formulation
                (smplx/loss/temporal_loss.py:121-131, 157-190: torch.spmm with lap_adj, gather of the nearest normals / vertices, relu, norms);
                the BASELINE, not the code under test, left as the reference writes it.  Both routes take the nearest body vertex from the
                package's search (fused.three_nn; chamferdist is not installed), per round, inside the timed region.
  (b) a whole step: PCALBSGarmentUseSegEncoderSeg.forward under grad (tuning.Tuning.refine_autograd: encoder, normals and skinning under
        no_grad, the head under grad), temporal_loss_PCA_LBS, total_loss.backward(), torch.optim.Adam.step() over the head's parameters.
Protocol of scripts/time_refine_grad.py: device events around each call after a warm-up; median and minimum.  One JSON line.
usage: python scripts/time_stage2_step.py [clips] [T] [side] [iters] [step: 0|1]      (Vg = side x side)"""
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from garment4d_amd import fused, gcn, losses, tuning
from garment4d_amd import synthetic as syn

clips = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 30
side = int(sys.argv[3]) if len(sys.argv) > 3 else 64
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 7
with_step = (int(sys.argv[5]) if len(sys.argv) > 5 else 1) != 0
assert torch.cuda.is_available(), "time_stage2_step.py measures on the GPU"
F_, Vg, N = clips * T, side * side, 8192
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


# ---- (a) the objective alone: a body cylinder, garments placed around it (about half of the vertices penetrate), the template's Laplacian
rng = np.random.default_rng(0)
scene = syn.garment_scene(clips, T, N if with_step else 4, body_rc=(65, 106), garment_rc=(side, side), seed=1)
body = scene["body"]
body_np = scene["batch"]["smpl_vertices_torch"].reshape(F_, -1, 3)
V = body_np.shape[1]
normals_np = syn.vertex_normals(body_np, body["faces"])
sel = rng.integers(0, V, Vg)
rounds0 = [dev(syn.garment_around_body(rng, body_np, normals_np, sel)) for _ in range(3)]
target = dev((body_np[:, sel] + rng.normal(0.0, 0.01, (F_, Vg, 3))).astype(np.float32))
body_v, body_vn = dev(body_np), dev(normals_np)
import scipy.sparse as sp
adj_old = gcn.adjacency_old_from_faces(scene["template"][1], Vg)
lap_adj = gcn.sparse_mx_to_torch_sparse_tensor(sp.eye(Vg) - gcn.normalize(adj_old)).cuda().coalesce()


def hip_loss():
    rounds = [p.clone().requires_grad_(True) for p in rounds0]
    total = losses.stage2_loss(rounds, target, body_v, body_vn, lap_adj, clips, T, LAMBDAS)[0]
    return total, torch.autograd.grad(total, rounds)


def torch_loss():
    rounds = [p.clone().requires_grad_(True) for p in rounds0]
    l2 = lap = pen = 0
    for i, p in enumerate(rounds):
        l2 = l2 + ((p - target) ** 2).sum(-1).mean()
        if i == len(rounds) - 1:
            msre = torch.sqrt(((p - target) ** 2).sum(-1)).mean(-1)      # the metrics the reference computes on the way
        pl = torch.spmm(lap_adj, p.transpose(0, 1).reshape(-1, F_ * 3)).reshape(-1, F_, 3).transpose(0, 1)
        lap = lap + torch.norm(pl, p=2, dim=-1).mean()
        with torch.no_grad():
            idx = fused.three_nn(p.detach().contiguous(), body_v)[1][..., :1].long()
        ex = idx.expand(idx.size(0), idx.size(1), 3)
        pen = pen + torch.relu(-torch.mul(torch.gather(body_vn, 1, ex), p - torch.gather(body_v, 1, ex)).sum(-1)).mean()
    last = rounds[-1].reshape(clips, T, -1, 3)
    tmp = ((last[:, :-1] - last[:, 1:]) ** 2).sum(-1).sqrt().mean()
    total = l2 * LAMBDAS[0] + lap * LAMBDAS[1] + pen * LAMBDAS[2] + tmp * LAMBDAS[3]
    return total, torch.autograd.grad(total, rounds), msre


out = dict(shape=dict(clips=clips, T=T, frames=F_, Vg=Vg, body=V, rounds=3))
a, b = hip_loss(), torch_loss()
out["loss_total_hip"], out["loss_total_torch"] = float(a[0].detach()), float(b[0].detach())
out["loss_grad_max_abs_diff"] = max(float((x - y).abs().max()) for x, y in zip(a[1], b[1]))
out["loss_grad_max_abs"] = max(float(y.abs().max()) for y in b[1])
del a, b
out["loss_hip_ms"], out["loss_hip_min_ms"] = timed(hip_loss)
out["loss_torch_ms"], out["loss_torch_min_ms"] = timed(torch_loss)
out["loss_speedup"] = out["loss_torch_ms"] / out["loss_hip_ms"]


def search_only():
    for p in rounds0:
        fused.three_nn(p, body_v)


out["three_nn_x3_ms"] = timed(search_only)[0]     # the share of both routes that is the (shared) nearest-vertex search
torch.cuda.empty_cache()

# ---- (b) a whole step
if with_step:
    from garment4d_amd.encoder import seed_encoder
    from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSeg, label_dict
    m = PCALBSGarmentUseSegEncoderSeg(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"], lbs_k=256, iteration=3)
    seed_encoder(m.PCA_garment_encoder, 0)
    with torch.no_grad():   # as scripts/time_model.py: untrained offset regressors would throw the garment away from the body
        for name, p in m.named_parameters():
            if not name.startswith("PCA_garment_encoder."):
                p.mul_(0.02 if name.startswith("lbs_graph_regress") and name.split(".")[1] == "3" else 0.5)
    m = m.cuda().eval()
    m.PCA_garment_encoder.channel_major_outputs = False
    x = dev(scene["x"])
    batch = {k: dev(v) for k, v in scene["batch"].items()}
    bm = types.SimpleNamespace(parents=torch.from_numpy(body["parents"]).cuda(), faces=body["faces"], J_regressor=dev(body["J_regressor"]),
                               v_template=dev(body["v_template"]))
    with torch.no_grad():
        logits = m.PCA_garment_encoder.pointnet.forward_fused(x.reshape(-1, N, 3))[1]
        tgt = label_dict["Tshirt"] - 1
        others = torch.cat([logits[..., :tgt], logits[..., tgt + 1:]], -1).max(-1)[0]
        m.PCA_garment_encoder.pointnet.FC_layer[2].conv.bias[tgt] += torch.quantile((others - logits[..., tgt]).flatten()[:1000000], 0.35)
        del logits, others
        posed = m(x, bm, batch)["lbs_pred_garment_v"]
    root = dev(rng.normal(0.0, 0.05, (clips, T, 3)).astype(np.float32))
    inputs = dict(pose_torch=batch["pose_torch"], smpl_vertices_torch=batch["smpl_vertices_torch"], smpl_root_joints_torch=root,
                  garment_torch=posed.reshape(clips, T, Vg, 3) + torch.randn(clips, T, Vg, 3, device="cuda") * 0.01 - root[:, :, None, :])
    head_params = [p for n, p in m.named_parameters() if not n.startswith("PCA_garment_encoder.")]
    opt = torch.optim.Adam(head_params, lr=1e-5)
    on = tuning.current().replace(refine_autograd=True)

    def forward_only():
        with torch.no_grad():
            return m(x, bm, batch)

    def step():
        opt.zero_grad(set_to_none=True)
        with tuning.use(on):
            od = m(x, bm, batch)
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
