"""Time the projective ray-depth loss (garment4d_amd/depth_fit.py) at the BASELINE cfg4 shape -- 240 frames (8 clips x 30), 4 ring cameras,
a sensor of 256 x 256 rays -- on the joined mesh of synthetic.garment_scene (body 6890 vertices + garment 4096, faces joined as render.render_output
joins them), next to what the parent commit offers for the same frames:
  (a) forward + backward of depth_mesh_distance, split into projection + rasterization (depth_fit.views) and the new kernels (terms, gradient);
  (b) the same frames through fit.point_mesh_distance on scan.scan_meshes clouds of 2048 and of 8192 points;
  (c) the same objective as device torch ops + autograd from the same face_id (fp32), and in float64 as the reference of both gradients' errors;
  (d) one step of each depth fit next to one step of each scan fit, also per entry point (garment: the scene's; body: the closed quad-cylinder
      body of scripts/time_smpl_grad.py, 6890 vertices, once at that script's parameters -- a torn surface, faces spanning tens of rays --
      and once as the smooth template).
Protocol: HIP events around each call after two warm-up runs; the median of `iters` (and the minimum).  One JSON line.
usage: python scripts/time_depth_fit.py [clips] [T] [image] [iters] [K]"""
import atexit
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from garment4d_amd import _lib, body_fit, depth_fit, fit, garment_fit, render, scan
from garment4d_amd import synthetic as syn
from garment4d_amd.body_models import SMPL, Struct
from garment4d_amd.mesh_encoder import PCALBSGarmentUseSegEncoderSeg

clips = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 30
SIZE = int(sys.argv[3]) if len(sys.argv) > 3 else 256
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 5
K = int(sys.argv[5]) if len(sys.argv) > 5 else 256
assert torch.cuda.is_available(), "time_depth_fit.py measures on the GPU"
TRUNC, GRAZING, LABEL = 0.05, 0.1, 6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def timed(fn):
    """Median and minimum of `iters` runs of fn() in microseconds, after two warm-up runs."""
    out = []
    for i in range(iters + 2):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            out.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": round(float(np.median(out)), 1), "min_us": round(float(np.min(out)), 1)}


def by_entry_point(fn):
    """Device microseconds of one fn() per C-ABI entry point (events around every call: _lib.timed_calls), largest first."""
    fn()
    with _lib.timed_calls() as t:
        fn()
    acc = {}
    for name, _, us in t.results():
        acc[name] = acc.get(name, 0.0) + us
    return {k: round(v, 1) for k, v in sorted(acc.items(), key=lambda kv: -kv[1])}


rng = np.random.default_rng(2)
scene = syn.garment_scene(clips, T, 4, body_rc=(65, 106), garment_rc=(64, 64), seed=1)
gv, gq = scene["template"]
Vg, F_ = gv.shape[0], clips * T
b = {k: dev(v) for k, v in scene["batch"].items()}
parents = torch.from_numpy(scene["body"]["parents"]).cuda()
body_model = types.SimpleNamespace(parents=parents, faces=scene["body"]["faces"])
gfaces = np.concatenate([gq[:, [0, 1, 2]], gq[:, [0, 2, 3]]], 0).astype(np.int64)
model = PCALBSGarmentUseSegEncoderSeg(garment_name="Tshirt", pca_dim=64, pca=scene["pca"], template=scene["template"], lbs_k=K, iteration=1).cuda().eval()
batch = dict(b, smpl_root_joints_torch=dev(rng.standard_normal((clips, T, 3)) * 0.05))
cams = scan.ring_cameras(4)
Vb = int(b["smpl_vertices_torch"].shape[2])
faces = render._joined_faces(body_model.faces, gfaces, Vb)
face_labels = torch.from_numpy(np.concatenate([np.zeros(len(body_model.faces), np.int32), np.full(len(gfaces), LABEL, np.int32)])).cuda()
coeff_true = dev(rng.standard_normal((clips, 64)) * 0.5)
coeff = (coeff_true + 0.3 * dev(rng.standard_normal((clips, 64)))).requires_grad_(True)


def joined(c):
    with torch.no_grad():
        posed = model.skin_garment(model.PCA_garment_encoder.PCA_inverse_transform(c), body_model, batch)[0].reshape(F_, Vg, 3)
        return torch.cat([b["smpl_vertices_torch"].reshape(F_, Vb, 3), posed + batch["smpl_root_joints_torch"].reshape(F_, 1, 3)], 1).contiguous()


target, verts = joined(coeff_true), joined(coeff.detach())
sensor = depth_fit.sensor_depth(target, faces, cams, SIZE, face_labels)
res = {"shape": {"frames": F_, "cams": len(cams), "image": SIZE, "V": int(verts.shape[1]), "faces": int(len(faces)), "K": K}, "iters": iters,
       "rays_hit_share": round(float((sensor.face_id >= 0).float().mean()), 4)}
atexit.register(lambda: print(json.dumps(res)))   # whatever was measured is printed, also when a later part fails

# (a) the depth term on the mesh itself
f_dev = render._faces(faces, verts.device)[0]
table = fit.vertex_corner_table(faces, int(verts.shape[1]), verts.device)
one = torch.ones(1, device="cuda")
res["raster_4_cameras"] = timed(lambda: depth_fit.views(verts, faces, cams, SIZE, SIZE))
s = depth_fit.views(verts, faces, cams, SIZE, SIZE)
res["depth_terms"] = timed(lambda: depth_fit.depth_terms(s, f_dev, sensor.depth, None, sensor.labels, face_labels, TRUNC, GRAZING))
terms = depth_fit.depth_terms(s, f_dev, sensor.depth, None, sensor.labels, face_labels, TRUNC, GRAZING, want_resid=True)
res["depth_vertex_grad"] = timed(lambda: depth_fit.depth_vertex_gradient(s, f_dev, sensor.depth, terms.total, one, table, None, sensor.labels, face_labels, TRUNC, GRAZING))
res["inliers_per_frame"] = round(float(terms.count.float().mean()), 1)
res["faces_with_an_inlier_share"] = round(float(torch.unique(s.face_id[~torch.isnan(terms.resid)]).numel()) / len(faces), 4)


def depth_whole():
    v = verts.detach().requires_grad_(True)
    depth_fit.depth_mesh_distance(sensor.depth, v, faces, cams, None, TRUNC, GRAZING, sensor.labels, face_labels).loss.backward()
    return v.grad


res["depth_mesh_distance_forward_backward"] = timed(depth_whole)
g_hip = depth_whole()
res["new_kernels_over_raster"] = round((res["depth_terms"]["median_us"] + res["depth_vertex_grad"]["median_us"]) / res["raster_4_cameras"]["median_us"], 3)

# (b) the same frames as clouds: the parent commit's data term
for n_points in (2048, 8192):
    cloud = scan.scan_meshes(target, faces, cams, SIZE, n_points, face_labels)
    res[f"scan_meshes_{n_points}"] = timed(lambda: scan.scan_meshes(target, faces, cams, SIZE, n_points, face_labels))

    def cloud_whole():
        v = verts.detach().requires_grad_(True)
        fit.point_mesh_distance(cloud.points, v, faces, None, TRUNC).loss.backward()

    res[f"point_mesh_distance_forward_backward_{n_points}"] = timed(cloud_whole)
    res[f"depth_speedup_over_cloud_{n_points}"] = round(res[f"point_mesh_distance_forward_backward_{n_points}"]["median_us"]
                                                        / res["depth_mesh_distance_forward_backward"]["median_us"], 2)

# (c) the same objective as torch ops + autograd from the same face_id and the same inlier set
inl = ~torch.isnan(terms.resid)
tri = f_dev.long()[s.face_id.clamp_min(0).long()]                                             # (K,F,h,w,3)
Rs = torch.from_numpy(s.cams_host[:, :9].reshape(-1, 3, 3).copy()).double().cuda()            # the projection's fp32 constants
eyes = torch.tensor([c.eye for c in cams], dtype=torch.float32).double().cuda()
ss = torch.from_numpy(s.cams_host[:, 9].copy()).double().cuda()
jj, ii = torch.meshgrid(torch.arange(SIZE, device="cuda"), torch.arange(SIZE, device="cuda"), indexing="xy")


def torch_loss(v, dt):
    total = torch.zeros((), dtype=dt, device="cuda")
    for c in range(len(cams)):
        cam = (v.to(dt) - eyes[c].to(dt)) @ Rs[c].to(dt).T                                    # (F,V,3)
        corner = torch.gather(cam, 1, tri[c].reshape(F_, -1, 1).expand(-1, -1, 3)).reshape(F_, SIZE, SIZE, 3, 3)
        c0, e1, e2 = corner[..., 0, :], corner[..., 1, :] - corner[..., 0, :], corner[..., 2, :] - corner[..., 0, :]
        n = torch.cross(e1, e2, dim=-1)
        shh = ss[c].to(dt) * (128 * SIZE)
        d = torch.stack([(256 * jj + 128 - 128 * SIZE).to(dt) / shh, (128 * SIZE - (256 * ii + 128)).to(dt) / shh, torch.ones_like(jj, dtype=dt)], -1)
        den = torch.where(inl[c], (n * d).sum(-1), torch.ones_like(d[..., 0]))              # (no 0 * inf in the backward of the masked terms)
        r = (n * c0).sum(-1) / den - torch.where(inl[c], sensor.depth[c], torch.zeros_like(sensor.depth[c])).to(dt)
        total = total + torch.where(inl[c], r * r, torch.zeros_like(r)).sum()
    return total / terms.total[0].to(dt)


def torch_whole(dt=torch.float32):
    v = verts.detach().requires_grad_(True)
    loss = torch_loss(v, dt)
    loss.backward()
    return loss.detach(), v.grad


res["torch_ops_forward_backward"] = timed(torch_whole)
res["torch_ops_over_depth_mesh_distance"] = round(res["torch_ops_forward_backward"]["median_us"] / res["depth_mesh_distance_forward_backward"]["median_us"], 2)
(l32, g32), (l64, g64) = torch_whole(), torch_whole(torch.float64)
scale = float(g64.abs().max())
res["loss"] = float(terms.total[1])
res["loss_rel_diff_vs_float64"] = abs(float(terms.total[1]) - float(l64)) / float(l64)
res["grad_err_hip_over_max"] = float((g_hip.double() - g64).abs().max()) / scale
res["grad_err_torch_fp32_over_max"] = float((g32.double() - g64).abs().max()) / scale
res["grad_err_ratio_hip_over_torch"] = round(res["grad_err_hip_over_max"] / res["grad_err_torch_fp32_over_max"], 3)
res["hip_grad_two_runs_same_bits"] = bool(torch.equal(depth_whole(), g_hip))
res["torch_grad_two_runs_same_bits"] = bool(torch.equal(torch_whole()[1], g32))

# (d) one step of each fit: garment
wt = (sensor.labels == LABEL).float()
cloud = scan.scan_meshes(target, faces, cams, SIZE, 2048, face_labels)
cw = (cloud.labels == LABEL).float()


def garment_depth_step():
    coeff.grad = None
    garment_fit.depth_garment_fit_loss(model, body_model, batch, coeff, sensor.depth, sensor.labels, cams, gfaces, LABEL, weights=wt, trunc=TRUNC)["total"].backward()


def garment_scan_step():
    coeff.grad = None
    garment_fit.garment_fit_loss(model, body_model, batch, coeff, cloud.points, cw, gfaces, trunc=TRUNC)["total"].backward()


res["garment_fit_step_depth"] = timed(garment_depth_step)
res["garment_fit_step_scan_2048"] = timed(garment_scan_step)
res["garment_fit_step_depth_by_entry_point"] = by_entry_point(garment_depth_step)
res["garment_fit_step_scan_by_entry_point"] = by_entry_point(garment_scan_step)
res["garment_fit_step_speedup"] = round(res["garment_fit_step_scan_2048"]["median_us"] / res["garment_fit_step_depth"]["median_us"], 2)

# (d) body: the closed quad-cylinder body of scripts/time_smpl_grad.py
V, J, NB = 6890, 24, 10
P = syn.smpl_like_params(V=V, J=J, num_betas=NB, seed=1)
betas_np, pose_np = syn.smpl_like_pose(F_, J=J, num_betas=NB, seed=2)
side = next(r for r in range(int(V ** 0.5), 1, -1) if V % r == 0)
cyl, quads = syn.quad_cylinder(side, V // side)
bfaces = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 0).astype(np.int64)
body = SMPL("", data_struct=Struct(**syn.smpl_data_struct(dict(P, v_template=cyl), bfaces)), gender="female", num_betas=NB, create_betas=False,
            create_global_orient=False, create_body_pose=False, create_transl=False).cuda()
bcams = scan.ring_cameras(4, distance=3.0)


def box_samples(v):
    """Mean number of samples in a face's sample box under the first camera: what the gradient's lanes walk per face."""
    p = render.project(v, bcams[0], SIZE, 1)
    f = render._faces(body.faces, v.device)[0].long()
    x, y = p.px[:, f].float() / 256, p.py[:, f].float() / 256                              # (F,nf,3)
    return round(float(((x.amax(-1) - x.amin(-1)) * (y.amax(-1) - y.amin(-1))).mean()), 2)


# "posed": the parameters of scripts/time_smpl_grad.py -- smpl_like_params' random shape and skinning directions tear the surface into long
# overlapping faces; "smooth": the template itself (betas = pose = 0), faces of about a sample
for tag, scale, off in (("", 1.0, (0.1, 0.01, 0.005)), ("_smooth", 0.0, (0.001, 0.001, 0.005))):
    betas, pose, transl = dev(betas_np * scale), dev(pose_np * scale), dev(np.zeros((F_, 3)))
    with torch.no_grad():
        bverts = body(betas=betas, global_orient=pose[:, :3], body_pose=pose[:, 3:], transl=transl).vertices
    bdepth = depth_fit.sensor_depth(bverts, body.faces, bcams, SIZE).depth
    bcloud = scan.scan_meshes(bverts, body.faces, bcams, SIZE, 2048).points
    start = (betas + off[0], pose + off[1], transl + off[2])
    res["body_rays_hit_share" + tag] = round(float(torch.isfinite(bdepth).float().mean()), 4)
    res["body_box_samples_per_face" + tag] = box_samples(bverts)

    def body_depth_step():
        bb, p, t = (x.detach().requires_grad_(True) for x in start)
        body_fit.depth_body_fit_loss(body, bb, p, t, bdepth, bcams, None, trunc=TRUNC)["total"].backward()

    def body_scan_step():
        bb, p, t = (x.detach().requires_grad_(True) for x in start)
        body_fit.body_fit_loss(body, bb, p, t, bcloud, None, trunc=TRUNC)["total"].backward()

    res["body_fit_step_depth" + tag] = timed(body_depth_step)
    res["body_fit_step_scan_2048" + tag] = timed(body_scan_step)
    res["body_fit_step_depth_by_entry_point" + tag] = by_entry_point(body_depth_step)
    res["body_fit_step_scan_by_entry_point" + tag] = by_entry_point(body_scan_step)
    res["body_fit_step_speedup" + tag] = round(res["body_fit_step_scan_2048" + tag]["median_us"] / res["body_fit_step_depth" + tag]["median_us"], 2)
