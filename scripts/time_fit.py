"""Time the point-to-surface loss (garment4d_amd/fit.py) at the BASELINE cfg4 shape: 240 frames (8 clips x 30), P = 8192 points per frame, half
of them labelled garment (weight 1) and half body (weight 0), against a 64 x 64 quad-cylinder garment split into triangles (4096 vertices,
8064 faces).
usage: python scripts/time_fit.py [frames] [iters] [points]

Prints device times (HIP events, median of `iters` after a warm-up) of the search (pre-pass + g4d_mesh_nearest_f32) over all points and
over the garment-labelled half alone -- the difference is what the search spends on weight-0 points --, of the forward, the grouping and the
gradient launches separately, of the whole point_mesh_distance(...).loss.backward(), and of the same objective written as device torch ops from
the same search result (gathers, the region classification as torch.where, autograd with its index_add_ adjoint): the baseline.
The last line is one JSON object with every figure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from garment4d_amd import fit, postprocess as pp, synthetic as syn

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 240
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
P = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
GARMENT_RC, TRUNC = (64, 64), 0.05


def tris(quads):
    q = np.asarray(quads)
    return np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)


def pose(verts, frame):
    v = np.asarray(verts, dtype=np.float64).copy()
    phase = 2 * np.pi * frame / 30.0
    v[:, 0] += 0.05 * np.sin(phase) * np.sin(np.pi * v[:, 1])
    v[:, 2] += 0.03 * np.cos(phase) * v[:, 1] ** 2
    return v.astype(np.float32)


def timed(fn):
    """Median device time of fn() in ms over `iters` runs after a warm-up, and its last result."""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), out


def torch_terms(q, a, b, c):
    """include/g4d.h's closest point on a triangle in torch ops (plain sums for the dot products): (point, dist2)."""
    ab, ac = b - a, c - a
    dot = lambda x, y: (x * y).sum(-1)
    d1, d2, d3, d4, d5, d6 = dot(ab, q - a), dot(ac, q - a), dot(ab, q - b), dot(ac, q - b), dot(ab, q - c), dot(ac, q - c)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & (e43 >= 0) & (e56 >= 0)]
    part = torch.zeros_like(d1, dtype=torch.int32)
    for cond, code in reversed(list(zip(conds, (4, 5, 1, 6, 3, 2)))):
        part = torch.where(cond, torch.full_like(part, code), part)
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    den = torch.where(part == 0, (va + vb) + vc, torch.where(part == 1, d1 - d3, torch.where(part == 2, e43 + e56, torch.where(part == 3, d2 - d6, one))))
    r = 1.0 / den
    w = torch.where(part == 0, vc * r, torch.where(part == 2, e43 * r, torch.where(part == 3, d2 * r, torch.where(part == 6, one, zero))))
    v = torch.where(part == 0, vb * r, torch.where(part == 1, d1 * r, torch.where(part == 2, 1.0 - w, torch.where(part == 5, one, zero))))
    point = a + ab * v[..., None] + ac * w[..., None]
    return point, ((q - point) ** 2).sum(-1)


def torch_loss(points, verts, faces_dev, face, weights, tau2):
    """The same objective as device torch ops under autograd: the adjoint to `verts` is the index_add_ behind the gathers (atomics)."""
    F_, n, _ = points.shape
    tri = faces_dev.long()[face.clamp_min(0).long()]                                       # (F, P, 3)
    corners = torch.gather(verts, 1, tri.reshape(F_, n * 3, 1).expand(-1, -1, 3)).reshape(F_, n, 3, 3)
    _, d2 = torch_terms(points, corners[:, :, 0], corners[:, :, 1], corners[:, :, 2])
    inlier = (face >= 0) & (weights > 0) & (d2 < tau2)
    return torch.where(inlier, weights * d2, torch.zeros_like(d2)).sum() / weights.sum()


assert torch.cuda.is_available(), "time_fit.py measures on the GPU; there is no CPU fallback"
rng = np.random.default_rng(1)
gv0, gq = syn.quad_cylinder(*GARMENT_RC)
faces = tris(gq)
garment_np = np.stack([pose(gv0, f) for f in range(frames)])
normals = syn.vertex_normals(garment_np, faces)
half = P // 2
# the garment-labelled half: garment-surface points (a vertex moved towards a random neighbour of its face and off the surface by N(0, 0.01));
# the body-labelled half: the same surface shrunk towards its axis by 15 %, the body under the garment
pick = rng.integers(0, len(faces), (frames, half))
bc = rng.dirichlet([1.0, 1.0, 1.0], (frames, half)).astype(np.float32)
rows = np.arange(frames)[:, None]
tri_v = garment_np[rows[..., None], faces[pick]]                                            # (F, half, 3, 3)
tri_n = normals[rows[..., None], faces[pick]].mean(2)
cloth = (bc[..., None] * tri_v).sum(2) + tri_n * rng.normal(0.0, 0.01, (frames, half, 1)).astype(np.float32)
axis = garment_np.mean(1, keepdims=True) * np.array([1.0, 0.0, 1.0], np.float32)
body_pts = garment_np[rows, rng.integers(0, garment_np.shape[1], (frames, P - half))]
body_pts = axis + (body_pts - axis) * np.array([0.85, 1.0, 0.85], np.float32) + rng.normal(0.0, 0.004, (frames, P - half, 3)).astype(np.float32)
points_np = np.concatenate([cloth, body_pts], 1).astype(np.float32)
weights_np = np.concatenate([np.ones((frames, half), np.float32), np.zeros((frames, P - half), np.float32)], 1)
perm = rng.permutation(P)
points_np, weights_np = np.ascontiguousarray(points_np[:, perm]), np.ascontiguousarray(weights_np[:, perm])

points, verts, weights = torch.from_numpy(points_np).cuda(), torch.from_numpy(garment_np).cuda(), torch.from_numpy(weights_np).cuda()
garment_pts = torch.from_numpy(np.ascontiguousarray(cloth.astype(np.float32))).cuda()
F_, V, nf = frames, verts.shape[1], len(faces)
tau2 = fit._tau2(TRUNC)
res = dict(frames=F_, points=P, garment_labelled=half, V=V, faces=nf, point_triangle_tests=F_ * P * nf)

res["search_prepass_ms"], mesh = timed(lambda: pp._SearchMesh(verts, faces))
res["search_all_points_ms"], near = timed(lambda: mesh.nearest(points))
res["search_garment_points_only_ms"], _ = timed(lambda: mesh.nearest(garment_pts))
res["search_share_spent_on_weight0_points"] = 1.0 - res["search_garment_points_only_ms"] / res["search_all_points_ms"]
faces_dev, table = mesh.topo["faces"], fit.vertex_corner_table(faces, V, verts.device)
res["forward_ms"], terms = timed(lambda: fit.point_face_terms(points, verts, faces_dev, near.face, weights, tau2))
res["group_ms"], keys = timed(lambda: fit.group_by_face(near.face, terms.inlier, nf))
one = torch.ones(1, device="cuda")
res["gradient_verts_ms"], (gv, _) = timed(lambda: fit.vertex_gradient(terms, keys, one, table, V, weights))
res["gradient_verts_and_points_ms"], (_, gp) = timed(lambda: fit.vertex_gradient(terms, keys, one, table, V, weights, want_points=True))
res["inlier_share_of_garment_points"] = float(terms.count.sum()) / (F_ * half)
res["loss"] = float(terms.total[1])
res["new_launches_ms"] = res["forward_ms"] + res["group_ms"] + res["gradient_verts_ms"]
res["new_launches_over_search"] = res["new_launches_ms"] / (res["search_prepass_ms"] + res["search_all_points_ms"])


def whole():
    v = verts.detach().requires_grad_(True)
    fit.point_mesh_distance(points, v, faces, weights, TRUNC).loss.backward()
    return v.grad


res["point_mesh_distance_backward_ms"], g_whole = timed(whole)
assert torch.equal(g_whole, gv), "the autograd route differs from the functional calls"


def torch_whole():
    v = verts.detach().requires_grad_(True)
    loss = torch_loss(points, v, faces_dev, near.face, weights, tau2)
    loss.backward()
    return loss.detach(), v.grad


res["torch_ops_forward_backward_ms"], (t_loss, t_grad) = timed(torch_whole)
res["torch_ops_over_new_launches"] = res["torch_ops_forward_backward_ms"] / res["new_launches_ms"]
res["torch_loss_rel_diff"] = abs(float(t_loss) - res["loss"]) / res["loss"]
res["torch_grad_max_abs_diff_over_max"] = float((t_grad - gv).abs().max() / gv.abs().max())
_, t_grad2 = torch_whole()
res["torch_grad_two_runs_same_bits"] = bool(torch.equal(t_grad, t_grad2))
res["hip_grad_two_runs_same_bits"] = bool(torch.equal(whole(), g_whole))
for k, v in res.items():
    print(f"{k}: {v}")
print(json.dumps(res))
