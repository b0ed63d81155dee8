"""Time the adjoint of the garment skinning at the cfg4 shape (8 clips x 30 frames = 240 frames, Vg 4096, V 6890, K 256, J 24) on one GPU, for both
weight routes -- materialised per-frame tables and the loader's stride-0 views (one table per clip):
  (a) each new call alone: g4d_garment_skin_grad_f32 over the clip's frames and for the un-posing, g4d_knn_blend_grad_f32 over the K list and
      over its 64-prefix, and the transposed smoothing (g4d_jacobi_smooth_f32 on the transposed operator);
  (b) forward, and forward + backward, through lbs_garment_interpolation under tuning.Tuning.garment_lbs_autograd;
  (c) the same computation as device torch ops + torch's autograd in the reference's form (reciprocal, masked assignment, gather, 100 sparse
      products, matmul; fp32) on the same GPU.  The BASELINE, not the code under test.  On the per-frame route it gathers in chunks of frames
      under checkpoint-free autograd and may need tens of GB; pass a smaller T to fit a smaller card;
  (d) one garment_fit.garment_fit_loss(...)['total'].backward() with P points per frame, and the nearest-face search of its forward alone.
Protocol: HIP events around each call after two warm-up runs; the median of `iters` (and the minimum).  One JSON line.
usage: python scripts/time_garment_fit.py [clips] [T] [P] [iters] [K]"""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from garment4d_amd import garment_fit, garment_lbs as GL, gcn, grad_ops, postprocess, tuning
from garment4d_amd import synthetic as syn
from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSeg

clips = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 30
P_ = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 5
K = int(sys.argv[5]) if len(sys.argv) > 5 else 256
assert torch.cuda.is_available(), "time_garment_fit.py measures on the GPU"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def timed(fn, setup=None):
    """Median and minimum of `iters` runs of fn(setup()) in microseconds, after two warm-up runs; setup runs outside the events."""
    out = []
    for i in range(iters + 2):
        arg = setup() if setup else None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(arg) if setup else fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            out.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": round(float(np.median(out)), 1), "min_us": round(float(np.min(out)), 1)}


scene = syn.garment_scene(clips, T, 4, body_rc=(65, 106), garment_rc=(64, 64), seed=1)
gv, gq = scene["template"]
Vg, F_ = gv.shape[0], clips * T
adj_old = gcn.adjacency_old_from_faces(gq, Vg)
b = {k: dev(v) for k, v in scene["batch"].items()}
parents = torch.from_numpy(scene["body"]["parents"]).cuda()
rng = np.random.default_rng(2)
x0 = dev(gv[None] + rng.standard_normal((clips, Vg, 3)) * 0.004)
dy = dev(rng.standard_normal((clips, T, Vg, 3)))
on = lambda: tuning.use(tuning.current().replace(garment_lbs_autograd=True))
res = {"shape": {"clips": clips, "T": T, "Vg": Vg, "V": int(b["T_lbs_weights"].shape[2]), "K": K, "J": int(b["T_lbs_weights"].shape[3]), "P": P_}, "iters": iters}


def tables(shared):
    Jr, W = b["T_J_regressor"], b["T_lbs_weights"]
    return (Jr[:, :1].expand(-1, T, -1, -1), W[:, :1].expand(-1, T, -1, -1)) if shared else (Jr, W)


def interp(x, shared):
    Jr, W = tables(shared)
    return GL.lbs_garment_interpolation(x, b["Tpose_smpl_vertices_torch"], b["Tpose_smpl_root_joints_torch"], b["zeropose_smpl_vertices_torch"], parents,
                                        b["pose_torch"], Jr, W, adj_old, K=K)


def torch_baseline(x, saved, shared):
    """The reference's formulation on the device, differentiable in x, the neighbour lists being the node's (constants)."""
    g0, body, idx_k, d_k, cW, inv_nn_W, inv_A, u0, Wt, nn_W0, A = saved
    idx = idx_k.long()
    J = cW.shape[2]
    K64 = min(64, K)
    bi = torch.arange(clips, device="cuda")[:, None, None]

    def weights(d):
        r = 1.0 / d
        r = torch.where(torch.isinf(r), torch.zeros_like(r), r)
        w = r / r.sum(-1, keepdim=True)
        return torch.where(torch.isinf(w), torch.zeros_like(w), w)

    def skin(W, A_, v):
        Tm = torch.matmul(W, A_.reshape(A_.shape[0], J, 16)).view(A_.shape[0], -1, 4, 4)
        return torch.matmul(Tm[..., :3, :3], v[..., None])[..., 0] + Tm[..., :3, 3]
    g = x + b["Tpose_smpl_root_joints_torch"].reshape(clips, 1, 3)
    d = ((g[:, :, None] - body[bi, idx]) ** 2).sum(-1)
    wK, w64 = weights(d), weights(d[..., :K64])
    u = skin((cW[bi, idx[..., :K64]] * w64[..., None]).sum(-2), inv_A, g)
    if shared:
        nn_W = (Wt[bi, idx] * wK[..., None]).sum(-2)
    else:
        nn_W = torch.stack([(Wt[c * T + t][idx[c]] * wK[c][..., None]).sum(-2) for c in range(clips) for t in range(T)])
    n = nn_W.shape[0]
    for _ in range(100):
        nn_W = nn_W + 0.1 * torch.sparse.mm(M_sparse, nn_W.transpose(0, 1).reshape(Vg, n * J)).reshape(Vg, n, J).transpose(0, 1)
    cl = torch.arange(F_, device="cuda") // T
    return skin(nn_W[cl] if shared else nn_W, A, u[cl])


import scipy.sparse as sp
m = sp.coo_matrix(sp.csr_matrix(gcn.normalize(adj_old) - sp.eye(Vg)))
M_sparse = torch.sparse_coo_tensor(torch.from_numpy(np.vstack((m.row, m.col)).astype(np.int64)), torch.from_numpy(m.data.astype(np.float32)), (Vg, Vg)).cuda().coalesce()

for shared in (False, True):
    r = {}
    with on():
        xr = x0.clone().requires_grad_(True)
        posed, _, stage1 = interp(xr, shared)
        saved = posed.grad_fn.saved_tensors
    g, body, idx_k, d_k, cW, inv_nn_W, inv_A, u, Wt, nn_W, A = saved
    r["saved_bytes"] = int(sum(t.numel() * t.element_size() for t in (g, idx_k, d_k, inv_nn_W, inv_A, u, nn_W, A)))
    dyf = dy.reshape(F_, Vg, 3)
    fpc = 1 if shared else T
    du, d_nn_W = grad_ops.garment_skin_grad(clips, T, nn_W, A, u, dyf)
    r["skin_grad_posing"] = timed(lambda: grad_ops.garment_skin_grad(clips, T, nn_W, A, u, dyf))
    r["smooth_transposed"] = timed(lambda: GL.smooth_weights(d_nn_W, adj_old, 0.1, 100, transpose=True))
    r["smooth_forward"] = timed(lambda: GL.smooth_weights(d_nn_W, adj_old, 0.1, 100))
    dW0 = GL.smooth_weights(d_nn_W, adj_old, 0.1, 100, transpose=True)
    r["blend_grad_K"] = timed(lambda: grad_ops.knn_blend_grad(Wt, fpc, idx_k, d_k, K, dW0, g, body))
    dg, d_inv_W = grad_ops.garment_skin_grad(clips, 1, inv_nn_W, inv_A, g, du)
    r["skin_grad_unposing"] = timed(lambda: grad_ops.garment_skin_grad(clips, 1, inv_nn_W, inv_A, g, du))
    r["blend_grad_K64"] = timed(lambda: grad_ops.knn_blend_grad(cW, 1, idx_k, d_k, min(64, K), d_inv_W, g, body, d_add=dg))
    with torch.no_grad():
        r["forward_flag_off"] = timed(lambda: interp(x0, shared))

    def fwd_bwd():
        with on():
            p = interp(xr, shared)[0]
        xr.grad = None
        p.backward(dy)
    r["forward_backward"] = timed(fwd_bwd)

    def base_fwd_bwd():
        xb = x0.clone().requires_grad_(True)
        torch_baseline(xb, saved, shared).backward(dyf)
    try:
        r["torch_forward_backward"] = timed(base_fwd_bwd)
        xb = x0.clone().requires_grad_(True)
        torch_baseline(xb, saved, shared).backward(dyf)
        fwd_bwd()
        r["max_abs_diff_vs_torch"] = float((xb.grad - xr.grad).abs().max())
        r["speedup_vs_torch"] = round(r["torch_forward_backward"]["median_us"] / r["forward_backward"]["median_us"], 1)
    except RuntimeError as e:   # out of memory on a small card: say so instead of a number
        r["torch_forward_backward"] = "failed: " + str(e).splitlines()[0][:120]
    res["shared_tables" if shared else "per_frame_tables"] = r
    del saved, posed, stage1
    torch.cuda.empty_cache()

# (d) one fit step on the vertices themselves (the model's own posing; K as above), and the share of its nearest-face search
model = PCALBSGarmentUseSegEncoderSeg(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"], lbs_k=K, iteration=1).cuda().eval()
body_model = types.SimpleNamespace(parents=parents, faces=scene["body"]["faces"])
faces = np.concatenate([gq[:, [0, 1, 2]], gq[:, [0, 2, 3]]], 0).astype(np.int64)
batch = dict(b, smpl_root_joints_torch=dev(rng.standard_normal((clips, T, 3)) * 0.05))
coeff = dev(rng.standard_normal((clips, 64)) * 0.5).requires_grad_(True)
with torch.no_grad():
    posed = model.skin_garment(model.PCA_garment_encoder.PCA_inverse_transform(coeff.detach()), body_model, batch)[0].reshape(F_, Vg, 3)
    posed = posed + batch["smpl_root_joints_torch"].reshape(F_, 1, 3)
    pts = (posed[:, torch.from_numpy(rng.integers(0, Vg, P_)).cuda()] + dev(rng.standard_normal((F_, P_, 3)) * 0.01)).contiguous()


def fit_step():
    coeff.grad = None
    garment_fit.garment_fit_loss(model, body_model, batch, coeff, pts, None, faces, trunc=0.05)["total"].backward()


res["fit_step"] = timed(fit_step)
ft = torch.from_numpy(faces).cuda()
with torch.no_grad():
    res["nearest_face_search"] = timed(lambda: postprocess.nearest_on_mesh(pts, posed, ft))
print(json.dumps(res))
