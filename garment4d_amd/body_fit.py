"""Register the SMPL body to a scan on HIP: the point-to-surface distance of the body-labelled points of a cloud to the body `body_model`
evaluates (fit.point_mesh_distance: exact nearest-face search, truncated, weighted, with its gradient to the vertices), carried on to betas,
pose and translation by the adjoint of lbs() (lbs.lbs_backward, csrc/smpl/smpl_grad.hip) -- the one input of the captured-data loop
(render.py, scan.py, fit.py) that used to come from outside: `inputs['pose_torch']` and the betas of every frame.

depth_body_fit_loss / fit_body_to_depth are the same fit for data that comes as depth images: the data term is depth_fit.depth_mesh_distance (the
association comes from rasterizing the current body from the sensors' cameras; no nearest-face search), everything else is unchanged.

Everything here needs tuning.Tuning.lbs_autograd for its gradients; the functions switch it on for their own calls of the body model and
leave the caller's setting alone.  fp32 on the current torch stream, no atomics, no host round trip inside fit_body_to_scan's loop.  There is no
fallback: without the libraries, or on CPU tensors, the calls raise."""
import torch

from . import depth_fit
from . import fit
from . import tuning


def _body_vertices(body_model, betas, pose, transl):
    """body_model(...) under the opt-in: pose (B, J*3) axis-angle, its first three numbers the global orientation."""
    if not (torch.is_tensor(pose) and pose.dim() == 2 and pose.shape[1] % 3 == 0 and pose.shape[1] >= 3):
        raise ValueError("body_fit: pose must be (B, J*3) axis-angle (global orientation first)")
    with tuning.use(tuning.current().replace(lbs_autograd=True)):
        return body_model(betas=betas, global_orient=pose[:, :3], body_pose=pose[:, 3:], transl=transl).vertices


def body_fit_loss(body_model, betas, pose, transl, points, weights, trunc=0.05, pose_prior=0.0, shape_prior=0.0):
    """betas (B,NB) or (1,NB), pose (B,J*3) axis-angle, transl (B,3) or None, points (B,P,3), weights (B,P) >= 0 or None -> dict:
      data   fit.point_mesh_distance(points, verts, body_model.faces, weights, trunc).loss on verts = body_model(betas, pose, transl).vertices
      pose   pose_prior  * mean ||body pose||^2   (the pose without its first three numbers; mean over frames and entries)
      shape  shape_prior * mean ||betas||^2
      total  their sum
    plus 'rms' (B) and 'inliers' (B) int32 of the data term, detached.  total.backward() fills .grad of whichever of betas, pose, transl
    requires grad (and of `points`, if it does)."""
    verts = _body_vertices(body_model, betas, pose, transl)
    f = fit.point_mesh_distance(points, verts, body_model.faces, weights, trunc)
    pose_term = pose_prior * (pose[:, 3:] ** 2).mean() if pose.shape[1] > 3 else pose_prior * pose.sum() * 0
    shape_term = shape_prior * (betas ** 2).mean()
    return {"data": f.loss, "pose": pose_term, "shape": shape_term, "total": f.loss + pose_term + shape_term, "rms": f.rms, "inliers": f.inliers}


def scan_body_fit_loss(body_model, inputs, betas, pose, transl, body_label=0, trunc=0.05, pose_prior=0.0, shape_prior=0.0):
    """body_fit_loss on a batch in the loader's form: points = inputs['pcd_torch'] (nbatch,T,N,3), weights = (inputs['pcd_label_torch'] ==
    body_label) (scan.scan_batch labels the body 0), betas / pose / transl per frame, (nbatch*T, .).  The root-joint convention of
    fit.scan_fit_loss: the clouds carry the root offset -- scan.scan_batch scans the body as lbs() poses it, root joint at
    inputs['smpl_root_joints_torch'], and adds that offset to the garment only --, and so does the body `body_model` evaluates: nothing is added
    here.  Returns body_fit_loss's dict with 'rms' and 'inliers' as (nbatch,T)."""
    pcd, lab = inputs["pcd_torch"], inputs["pcd_label_torch"]
    if not (torch.is_tensor(pcd) and pcd.dim() == 4 and pcd.shape[-1] == 3):
        raise ValueError("scan_body_fit_loss: inputs['pcd_torch'] must be (nbatch, T, N, 3)")
    nbatch, T, N = (int(x) for x in pcd.shape[:3])
    if not (torch.is_tensor(lab) and lab.numel() == nbatch * T * N):
        raise ValueError("scan_body_fit_loss: inputs['pcd_label_torch'] (nbatch, T, N, 1) expected")
    if not (pcd.is_cuda and pcd.dtype == torch.float32):
        raise TypeError("scan_body_fit_loss: inputs['pcd_torch'] must be a float32 HIP tensor (no CPU fallback)")
    weights = (lab.reshape(nbatch * T, N) == int(body_label)).to(torch.float32)
    out = body_fit_loss(body_model, betas, pose, transl, pcd.reshape(nbatch * T, N, 3), weights, trunc, pose_prior, shape_prior)
    out["rms"], out["inliers"] = out["rms"].view(nbatch, T), out["inliers"].view(nbatch, T)
    return out


def fit_body_to_scan(body_model, points, weights, betas0, pose0, transl0, steps, lr, trunc=0.05, pose_prior=0.0, shape_prior=0.0):
    """`steps` steps of torch.optim.Adam(lr) on copies of (betas0, pose0, transl0), minimising body_fit_loss(...)['total']: a plain loop, no line
    search, no staged schedule, nothing read back to the host.  Returns (betas, pose, transl, losses): the fitted tensors (detached) and the
    device tensor of the steps + 1 totals -- before every step, and after the last."""
    betas, pose, transl = (t.detach().clone().requires_grad_(True) for t in (betas0, pose0, transl0))
    opt = torch.optim.Adam([betas, pose, transl], lr=lr)
    losses = torch.zeros(int(steps) + 1, dtype=torch.float32, device=points.device)
    for i in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        total = body_fit_loss(body_model, betas, pose, transl, points, weights, trunc, pose_prior, shape_prior)["total"]
        total.backward()
        losses[i] = total.detach()
        opt.step()
    with torch.no_grad():
        losses[int(steps)] = body_fit_loss(body_model, betas, pose, transl, points, weights, trunc, pose_prior, shape_prior)["total"]
    return betas.detach(), pose.detach(), transl.detach(), losses


def depth_body_fit_loss(body_model, betas, pose, transl, depth_obs, cameras, weights=None, trunc=0.05, grazing=0.1, pose_prior=0.0, shape_prior=0.0):
    """body_fit_loss for data that comes as depth images: depth_obs (K,B,h,w) of the K `cameras` (render.Camera), weights (K,B,h,w) >= 0 or None.
    The data term is depth_fit.depth_mesh_distance(depth_obs, verts, body_model.faces, cameras, weights, trunc, grazing).loss -- the association
    comes from rasterizing the current body, no nearest-face search --; the priors, the dict's keys and what total.backward() fills are
    body_fit_loss's."""
    verts = _body_vertices(body_model, betas, pose, transl)
    f = depth_fit.depth_mesh_distance(depth_obs, verts, body_model.faces, cameras, weights, trunc, grazing)
    pose_term = pose_prior * (pose[:, 3:] ** 2).mean() if pose.shape[1] > 3 else pose_prior * pose.sum() * 0
    shape_term = shape_prior * (betas ** 2).mean()
    return {"data": f.loss, "pose": pose_term, "shape": shape_term, "total": f.loss + pose_term + shape_term, "rms": f.rms, "inliers": f.inliers}


def fit_body_to_depth(body_model, depth_obs, cameras, weights, betas0, pose0, transl0, steps, lr, trunc=0.05, grazing=0.1, pose_prior=0.0,
                      shape_prior=0.0):
    """fit_body_to_scan's plain Adam loop on depth_body_fit_loss(...)['total']: the body is rasterized anew at every step.  Returns (betas, pose,
    transl, losses) as fit_body_to_scan does."""
    betas, pose, transl = (t.detach().clone().requires_grad_(True) for t in (betas0, pose0, transl0))
    opt = torch.optim.Adam([betas, pose, transl], lr=lr)
    losses = torch.zeros(int(steps) + 1, dtype=torch.float32, device=depth_obs.device)
    args = (depth_obs, cameras, weights, trunc, grazing, pose_prior, shape_prior)
    for i in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        total = depth_body_fit_loss(body_model, betas, pose, transl, *args)["total"]
        total.backward()
        losses[i] = total.detach()
        opt.step()
    with torch.no_grad():
        losses[int(steps)] = depth_body_fit_loss(body_model, betas, pose, transl, *args)["total"]
    return betas.detach(), pose.detach(), transl.detach(), losses
