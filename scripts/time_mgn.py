"""Time the MGN variant's skinning at the cfg4 shape (8 clips x 30 frames, Vg = 4096, V = 6890, J = 24) on one GPU:
  fused     g4d_mgn_skin_f32 alone (K = 1 search + both blends at the nearest vertex, inv_A / A given)
  lbs_MGN   the whole lbs_garment_MGN (Rodrigues, joints and rigid transforms from the lbs helpers + the fused launch)
  composed  the same search + blends from existing pieces in the reference's form: knn_points(K = 1) on the body repeated per frame,
            torch.matmul(W, inv_A) / torch.gather / torch.matmul (modules/mesh_encoder.py:541-583), inv_A / A given
  forward   PCALBSGarmentUseSegEncoderSegMGN.forward (encoder + displacement MLP + lbs_garment_MGN), N points per frame
Device events around `iters` calls after a warm-up; the median call is printed, plus the search rate in distance evaluations per second.
usage: python scripts/time_mgn.py [nbatch] [T] [N] [iters]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from garment4d_amd import _lib
from garment4d_amd import lbs as L
from garment4d_amd import synthetic as syn
from garment4d_amd.encoder import seed_encoder
from garment4d_amd.garment_lbs import lbs_garment_MGN
from garment4d_amd.knn import knn_points
from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSegMGN

nbatch = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 30
N = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 10
assert torch.cuda.is_available(), "time_mgn.py measures on the GPU"


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


scene = syn.garment_scene(nbatch, T, N, body_rc=(65, 106), garment_rc=(64, 64), seed=1)
b = {k: dev(v) for k, v in scene["batch"].items()}
gv = scene["template"][0]
Vg, V, J, F_ = gv.shape[0], scene["body"]["v_template"].shape[0], 24, nbatch * T
parents = torch.from_numpy(scene["body"]["parents"]).cuda()
rng = np.random.default_rng(3)
garment = dev((gv[None, None] + rng.standard_normal((nbatch, T, Vg, 3)) * 0.01).astype(np.float32))
body_model = type("BM", (), dict(parents=parents, faces=scene["body"]["faces"], J_regressor=dev(scene["body"]["J_regressor"])))()

# the transforms both the fused and the composed path consume (computed once, outside the timed region)
Jreg = b["T_J_regressor"].reshape(F_, J, V).contiguous()
body = b["Tpose_smpl_vertices_torch"].reshape(nbatch, V, 3).contiguous()
body_f = body.reshape(nbatch, 1, V, 3).expand(nbatch, T, V, 3).reshape(F_, V, 3).contiguous()
inv_pose = torch.zeros((F_, 24, 3), device="cuda")
inv_pose[:, 0, 0], inv_pose[:, 1, 1], inv_pose[:, 2, 1] = -np.pi / 2, 0.15, -0.15
_, inv_A = L.batch_rigid_transform(L.batch_rodrigues(inv_pose.reshape(-1, 3)).reshape(F_, 24, 3, 3), L.vertices2jointsB(Jreg, body_f), parents)
_, A = L.batch_rigid_transform(L.batch_rodrigues(b["pose_torch"].reshape(-1, 3)).reshape(F_, 24, 3, 3),
                               L.vertices2jointsB(Jreg, b["zeropose_smpl_vertices_torch"].reshape(F_, V, 3).contiguous()), parents)
W = b["T_lbs_weights"].reshape(F_, V, J).contiguous()
root = b["Tpose_smpl_root_joints_torch"].reshape(nbatch, 3).contiguous()
g_flat = garment.reshape(F_, Vg, 3).contiguous()
o_idx = torch.empty((F_, Vg), dtype=torch.int32, device="cuda")
o_d, o_s, o_p = torch.empty((F_, Vg), device="cuda"), torch.empty((F_, Vg, 3), device="cuda"), torch.empty((F_, Vg, 3), device="cuda")


def fused():
    _lib.call("g4d_mgn_skin_f32", nbatch, T, Vg, V, J, g_flat.data_ptr(), root.data_ptr(), body.data_ptr(), W.data_ptr(), inv_A.data_ptr(),
              A.data_ptr(), o_idx.data_ptr(), o_d.data_ptr(), o_s.data_ptr(), o_p.data_ptr(), _lib.stream_ptr())


def composed():
    """modules/mesh_encoder.py:538-583 with knn_points on the HIP K-nearest kernel and torch for the blends."""
    q = (garment + root.reshape(nbatch, 1, 1, 3)).reshape(F_, Vg, 3)
    new_T = body.reshape(nbatch, 1, V, 3).repeat(1, T, 1, 1).reshape(F_, V, 3)
    nn = knn_points(q, new_T, K=1)
    inv_T = torch.matmul(W, inv_A.view(F_, J, 16)).view(F_, V, 4, 4)
    inv_nn_T = torch.gather(inv_T, 1, nn.idx.reshape(F_, -1, 1, 1).repeat(1, 1, 4, 4))
    homo = torch.cat([q, torch.ones((F_, Vg, 1), device="cuda")], 2)
    s = torch.matmul(inv_nn_T, homo.unsqueeze(-1))[:, :, :3, 0]
    Tm = torch.matmul(W, A.view(F_, J, 16)).view(F_, V, 4, 4)
    nn_T = torch.gather(Tm, 1, nn.idx.reshape(F_, -1, 1, 1).repeat(1, 1, 4, 4))
    p = torch.matmul(nn_T, torch.cat([s, torch.ones((F_, Vg, 1), device="cuda")], 2).unsqueeze(-1))[:, :, :3, 0]
    return nn, s, p


def whole():
    return lbs_garment_MGN(garment, b["Tpose_smpl_vertices_torch"], b["Tpose_smpl_root_joints_torch"], b["zeropose_smpl_vertices_torch"], parents,
                           b["pose_torch"], b["T_J_regressor"], b["T_lbs_weights"], K=1)


with torch.no_grad():
    fused()
    nn_c, s_c, p_c = composed()
    torch.cuda.synchronize()
    agree = dict(idx_equal=bool(torch.equal(o_idx.long(), nn_c.idx[..., 0])), dist_equal=bool(torch.equal(o_d, nn_c.dists[..., 0])),
                 stage1_max_abs_diff=float((o_s - s_c).abs().max()), posed_max_abs_diff=float((o_p - p_c).abs().max()))
    res = dict(shape=dict(nbatch=nbatch, T=T, Vg=Vg, V=V, J=J, N=N), agreement=agree)
    res["fused_ms"] = timed(fused)[0]
    res["composed_ms"] = timed(composed)[0]
    res["lbs_garment_MGN_ms"] = timed(whole)[0]
    evals = F_ * Vg * V
    res["distance_evaluations"] = evals
    res["fused_Geval_per_s"] = evals / (res["fused_ms"] * 1e-3) / 1e9
    del nn_c, s_c, p_c
    torch.manual_seed(0)
    m = PCALBSGarmentUseSegEncoderSegMGN(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"])
    seed_encoder(m.PCA_garment_encoder, 0)
    m = m.cuda().eval()
    x = dev(scene["x"])
    res["forward_ms"] = timed(lambda: m(x, body_model, b), n=max(3, iters // 2))[0]
print(json.dumps(res))
