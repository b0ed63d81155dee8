"""Time the adjoint of lbs() at the cfg4 shape (B = 240 frames, V = 6890, J = 24, NB = 10) on one GPU:
  (a) lbs.lbs_backward alone (g4d_smpl_lbs_grad_f32: three launches), and forward + backward (lbs() under tuning.Tuning.lbs_autograd, then
      backward of given upstream gradients);
  (b) the same computation as device torch ops + torch's autograd in the reference's form (tests/smpl_grad_twin.torch_lbs, fp32) on the same
      GPU: backward alone and forward + backward.  The BASELINE, not the code under test;
  (c) one body_fit.body_fit_loss(...)['total'].backward() on a closed quad-cylinder body of 6890 vertices with P points per frame, and the
      nearest-face search of its forward alone (postprocess's exact search: the share of the step spent there);
  (d) the workspace bytes of (a).
Protocol: HIP events around each call after a warm-up; the median of 5 (and the minimum).  One JSON line.
usage: python scripts/time_smpl_grad.py [B] [V] [P] [iters]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import smpl_grad_twin as ST
from garment4d_amd import _lib, body_fit, postprocess, tuning
from garment4d_amd import lbs as L
from garment4d_amd import synthetic as syn
from garment4d_amd.body_models import SMPL, Struct

B = int(sys.argv[1]) if len(sys.argv) > 1 else 240
V = int(sys.argv[2]) if len(sys.argv) > 2 else 6890
P_ = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 5
assert torch.cuda.is_available(), "time_smpl_grad.py measures on the GPU"
J, NB = 24, 10


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


P = syn.smpl_like_params(V=V, J=J, num_betas=NB, seed=1)
betas_np, pose_np = syn.smpl_like_pose(B, J=J, num_betas=NB, seed=2)
rng = np.random.default_rng(3)
consts = (dev(P["v_template"]), dev(P["shapedirs"]), dev(P["posedirs"]), dev(P["J_regressor"]), torch.from_numpy(P["parents"]), dev(P["lbs_weights"]))
gv, gj = dev(rng.standard_normal((B, V, 3))), dev(rng.standard_normal((B, J, 3)))
res = {"shape": {"B": B, "V": V, "J": J, "NB": NB, "P": P_}, "iters": iters}

# (a) the HIP route
betas, pose = dev(betas_np), dev(pose_np)
res["hip_backward"] = timed(lambda: L.lbs_backward(betas, pose, *consts, gv, gj))
res["hip_forward"] = timed(lambda: L.lbs(betas, pose, *consts))
on = tuning.current().replace(lbs_autograd=True)


def hip_fb():
    b, p = betas.detach().requires_grad_(True), pose.detach().requires_grad_(True)
    with tuning.use(on):
        verts, joints = L.lbs(b, p, *consts)
    torch.autograd.backward([verts, joints], [gv, gj])


res["hip_forward_backward"] = timed(hip_fb)

# (b) torch ops + autograd, reference form, same GPU
tp = ST.torch_params(P, torch.float32, "cuda")


def torch_graph():
    b, p = betas.detach().requires_grad_(True), pose.detach().requires_grad_(True)
    return ST.torch_lbs(b, p, tp)


res["torch_backward"] = timed(lambda out: torch.autograd.backward(list(out), [gv, gj]), setup=torch_graph)
res["torch_forward_backward"] = timed(lambda: torch.autograd.backward(list(torch_graph()), [gv, gj]))

# (c) one step of the body fit
side = next(r for r in range(int(V ** 0.5), 1, -1) if V % r == 0)
cyl, quads = syn.quad_cylinder(side, V // side)
faces = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 0).astype(np.int64)
Pc = dict(P, v_template=cyl)
body = SMPL("", data_struct=Struct(**syn.smpl_data_struct(Pc, faces)), gender="female", num_betas=NB, create_betas=False, create_global_orient=False,
            create_body_pose=False, create_transl=False).cuda()
transl = dev(np.zeros((B, 3)))
with torch.no_grad():
    verts = body(betas=betas, global_orient=pose[:, :3], body_pose=pose[:, 3:], transl=transl).vertices
pick = torch.from_numpy(rng.integers(0, V, (B, P_))).cuda()
points = (torch.gather(verts, 1, pick[..., None].expand(-1, -1, 3)) + 0.005 * dev(rng.standard_normal((B, P_, 3)))).contiguous()


def fit_step():
    b, p, t = (x.detach().requires_grad_(True) for x in (betas, pose, transl))
    body_fit.body_fit_loss(body, b, p, t, points, None, trunc=0.05)["total"].backward()


res["body_fit_step"] = timed(fit_step)
mesh = postprocess._SearchMesh(verts, faces, None)
res["body_fit_search"] = timed(lambda: mesh.nearest(points))
res["body_fit_search_share"] = round(res["body_fit_search"]["median_us"] / res["body_fit_step"]["median_us"], 3)

# (d)
Ls = _lib.smpl_lib()[0]
res["workspace_bytes"] = int(Ls.g4d_smpl_grad_ws_bytes(B, V, J, NB))
res["slabs"] = int(Ls.g4d_smpl_grad_slabs(B, V))
res["hip_over_torch_backward"] = round(res["hip_backward"]["median_us"] / res["torch_backward"]["median_us"], 3)
print(json.dumps(res))
