"""Time the stage-1 objective, values + gradient w.r.t. (logits, PCA coefficients, T-pose garment), at the cfg4 shape (8 clips x 30 frames x 8192
points x 7 classes, 4096 garment / 6890 body vertices, batch size 8) on one GPU:
  hip     losses.stage1_loss: g4d_stage1_ce_f32 + g4d_stage1_garment_f32 (csrc/stage1_loss.hip) + the nearest-vertex search
  torch   (a) the same objective as plain device torch ops + torch's autograd: F.cross_entropy, the cotangents in the dot / cross form under
          no_grad, the Laplacian applied with index_add_ over the same (face, corner) incidences (L a constant of the graph)
  host    (b) the reference's form of the Laplacian term (smplx/loss/laplacian.py:199-265): the vertices copied to the host, a scipy CSR
          assembled from the cotangents, one sparse product, the result copied back -- twice per iteration (target and prediction), and a third
          product in the backward; everything else as in (a).  Written for this script; the BASELINE, not the code under test.
All three take the nearest body vertex from the package's search (fused.three_nn; chamferdist is not installed) inside the timed region; its
share is reported.  Per entry point: the device time of each C-ABI call (_lib.timed_calls).
Protocol of scripts/time_stage2_step.py: device events around each call after a warm-up; median and minimum.  One JSON line.
usage: python scripts/time_stage1_loss.py [clips] [T] [N] [side] [iters] [baselines: 0|1]      (Vg = side x side)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from garment4d_amd import _lib, fused, losses
from garment4d_amd import synthetic as syn

clips = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 30
N = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
side = int(sys.argv[4]) if len(sys.argv) > 4 else 64
iters = int(sys.argv[5]) if len(sys.argv) > 5 else 7
baselines = (int(sys.argv[6]) if len(sys.argv) > 6 else 1) != 0
assert torch.cuda.is_available(), "time_stage1_loss.py measures on the GPU"
C, P, Vg, Bp = 7, 64, side * side, clips
LAMBDAS = (0.05, 0.001, 40.0, 50.0, 1.0)            # cfgs/tshirt.yaml


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


# a T-pose body cylinder (6890 vertices), the garment template's own cylinder widened to sit around it, perturbed per clip
rng = np.random.default_rng(0)
scene = syn.garment_scene(clips, 1, 4, body_rc=(65, 106), garment_rc=(side, side), seed=1)
body_np = scene["batch"]["Tpose_smpl_vertices_torch"].reshape(clips, -1, 3)
V = body_np.shape[1]
normals_np = syn.vertex_normals(body_np, scene["body"]["faces"])
root_np = rng.normal(0.0, 0.05, (clips, 3)).astype(np.float32)
sel = rng.integers(0, V, Vg)
pred0 = dev(syn.garment_around_body(rng, body_np, normals_np, sel) - root_np[:, None, :])
target = dev((body_np[:, sel] + rng.normal(0.0, 0.03, (clips, Vg, 3))).astype(np.float32) - root_np[:, None, :])
body_v, body_vn, root = dev(body_np), dev(normals_np), dev(root_np)
quads = scene["template"][1]
faces3 = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
logits0 = dev((rng.standard_normal((clips * T, N, C)) * 2).astype(np.float32))
labels = dev(rng.integers(0, C, clips * T * N).astype(np.int64))
coeff0 = dev(rng.standard_normal((clips, P)).astype(np.float32))
coeff_gt = dev(rng.standard_normal((clips, P)).astype(np.float32))
f_dev = dev(faces3.astype(np.int64))


def leaves():
    return [t.clone().requires_grad_(True) for t in (logits0, coeff0, pred0)]


def hip_loss():
    lg, a, p = leaves()
    total = losses.stage1_loss(lg, labels, a, coeff_gt, p, target, root, body_v, body_vn, faces3, Bp, LAMBDAS)[0]
    return total, torch.autograd.grad(total, [lg, a, p])


def cotangents(x):
    """(B, nf, 3) half-cotangents per corner, zero on a face of zero area."""
    a, b, c = x[:, f_dev[:, 0]], x[:, f_dev[:, 1]], x[:, f_dev[:, 2]]
    ab, ac, bc = b - a, c - a, c - b
    n = torch.cross(ab, ac, dim=-1).norm(dim=-1, keepdim=True)
    d = torch.stack([(ab * ac).sum(-1), -(bc * ab).sum(-1), (ac * bc).sum(-1)], -1)
    return torch.where(n > 0, 0.5 * d / n, torch.zeros_like(d))


def lap_device(x, h):
    out = torch.zeros_like(x)
    for c in range(3):
        c1, c2 = (c + 1) % 3, (c + 2) % 3
        xi = x[:, f_dev[:, c]]
        out.index_add_(1, f_dev[:, c], h[:, :, c1, None] * (x[:, f_dev[:, c2]] - xi) + h[:, :, c2, None] * (x[:, f_dev[:, c1]] - xi))
    return out


class HostLaplacian(torch.autograd.Function):
    """L(x) x with L assembled and applied on the host, L x copied back; the backward is one more host product with the same L."""

    @staticmethod
    def forward(ctx, x):
        import scipy.sparse as sp
        B, n, _ = x.shape
        h = cotangents(x).cpu().numpy().reshape(-1, 3)
        xv = x.detach().cpu().numpy().reshape(-1, 3)
        f = (faces3[None].astype(np.int64) + (np.arange(B) * n)[:, None, None]).reshape(-1, 3)
        rows, cols = f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
        L = sp.csr_matrix((h.reshape(-1), (rows, cols)), shape=(B * n, B * n))
        L = L + L.T
        L = L - sp.diags(np.asarray(L.sum(1)).reshape(-1), format="csr")
        ctx.L = L
        return torch.from_numpy(np.asarray(L.dot(xv), dtype=np.float32).reshape(B, n, 3)).to(x.device)

    @staticmethod
    def backward(ctx, g):
        return torch.from_numpy(np.asarray(ctx.L.dot(g.cpu().numpy().reshape(-1, 3)), dtype=np.float32).reshape(g.shape)).to(g.device)


def torch_loss(host_laplacian=False):
    lg, a, p = leaves()
    sem = torch.nn.functional.cross_entropy(lg.reshape(-1, C), labels)
    pca = ((a - coeff_gt) ** 2).mean()
    l2 = ((p - target) ** 2).sum(-1).mean()
    msre = torch.sqrt(((p - target) ** 2).sum(-1)).mean()
    q = p + root[:, None, :]
    with torch.no_grad():
        idx = fused.three_nn(q.detach().contiguous(), body_v)[1][..., :1].long()
    ex = idx.expand(idx.size(0), idx.size(1), 3)
    pen = torch.relu(-torch.mul(torch.gather(body_vn, 1, ex), q - torch.gather(body_v, 1, ex)).sum(-1)).mean()
    if host_laplacian:
        cg, lp = HostLaplacian.apply(target).norm(dim=-1), HostLaplacian.apply(p)
    else:
        with torch.no_grad():
            cg, hp = lap_device(target, cotangents(target)).norm(dim=-1), cotangents(p)
        lp = lap_device(p, hp)
    lap = (lp.norm(dim=-1) - cg).abs().mean()          # (batch size = clips: no padding at this shape)
    total = sem * LAMBDAS[0] + pca * LAMBDAS[1] + l2 * LAMBDAS[2] + pen * LAMBDAS[3] + lap * LAMBDAS[4]
    return total, torch.autograd.grad(total, [lg, a, p]), msre


out = dict(shape=dict(clips=clips, T=T, N=N, classes=C, rows=clips * T * N, Vg=Vg, faces=int(faces3.shape[0]), body=V, pca=P, pad_batch=Bp))
a = hip_loss()
out["loss_total_hip"] = float(a[0].detach())
if baselines:
    b, c = torch_loss(), torch_loss(True)
    out["loss_total_torch"], out["loss_total_host"] = float(b[0].detach()), float(c[0].detach())
    out["grad_max_abs_diff_vs_torch"] = [float((x - y).abs().max()) for x, y in zip(a[1], b[1])]
    out["grad_max_abs"] = [float(y.abs().max()) for y in b[1]]
    del b, c
del a
out["loss_hip_ms"], out["loss_hip_min_ms"] = timed(hip_loss)
if baselines:
    out["loss_torch_ms"], out["loss_torch_min_ms"] = timed(torch_loss)
    out["loss_host_ms"], out["loss_host_min_ms"] = timed(lambda: torch_loss(True), n=max(3, iters // 2), warm=1)
    out["speedup_vs_torch"] = out["loss_torch_ms"] / out["loss_hip_ms"]
    out["speedup_vs_host"] = out["loss_host_ms"] / out["loss_hip_ms"]
q0 = (pred0 + root[:, None, :]).contiguous()
out["three_nn_ms"] = timed(lambda: fused.three_nn(q0, body_v))[0]     # the share of every route that is the (shared) nearest-vertex search
calls = {}
for _ in range(iters):
    with _lib.timed_calls() as t:
        hip_loss()
    for name, _ints, us in t.results():
        calls.setdefault(name, []).append(us)
out["calls_us"] = {k: float(np.median(v)) for k, v in calls.items()}
print(json.dumps(out))
