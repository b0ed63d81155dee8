"""Fit the garment to a scan on HIP: the point-to-surface distance of the garment-labelled points of a cloud to the garment the model poses
(fit.point_mesh_distance: exact nearest-face search, truncated, weighted, with its gradient to the vertices), carried back through the garment
skinning (garment_lbs.lbs_garment_interpolation's adjoint, csrc/skin/skin_grad.hip) to the T-pose garment and, through
PCAGarmentEncoderSeg.PCA_inverse_transform, to the PCA coefficients -- the last piece of the captured-data loop scan.py -> body_fit.py -> here.

depth_garment_fit_loss / fit_garment_to_depth are the same fit for data that comes as depth and label images: the data term is
depth_fit.depth_mesh_distance on the body joined with the posed garment, so the body occludes the garment as it does for the sensor.

Everything here needs tuning.Tuning.garment_lbs_autograd (and stage1_autograd for coefficients) for its gradients; the functions switch them on
for their own calls of the model and leave the caller's setting alone.  The body (pose, T-pose vertices, tables: `batch`) is a constant: joint
body + garment fitting is out of scope.  fp32 on the current torch stream, no atomics, no host round trip inside fit_garment_to_scan's loop.
There is no fallback: without the libraries, or on CPU tensors, the calls raise."""
import numpy as np
import torch

from . import _cache
from . import depth_fit
from . import fit
from . import render
from . import tuning


def _posed_garment(model, body_model, batch, coeff_or_verts):
    """coeff_or_verts (nbatch, pca_dim) PCA coefficients or (nbatch, Vg, 3) the T-pose garment itself -> (T-pose garment (nbatch,Vg,3), posed
    garment (nbatch,T,Vg,3)) under the two opt-ins."""
    if not (torch.is_tensor(coeff_or_verts) and coeff_or_verts.dim() in (2, 3)):
        raise ValueError("garment_fit: coeff_or_verts must be (nbatch, pca_dim) coefficients or (nbatch, Vg, 3) T-pose vertices")
    if coeff_or_verts.dim() == 3 and coeff_or_verts.shape[2] != 3:
        raise ValueError("garment_fit: T-pose vertices must be (nbatch, Vg, 3)")
    with tuning.use(tuning.current().replace(garment_lbs_autograd=True, stage1_autograd=True)):
        tpose = model.PCA_garment_encoder.PCA_inverse_transform(coeff_or_verts) if coeff_or_verts.dim() == 2 else coeff_or_verts
        posed, _, _ = model.skin_garment(tpose, body_model, batch)
    return tpose, posed


def garment_fit_loss(model, body_model, batch, coeff_or_verts, points, weights, garment_faces, trunc=0.05, coeff_prior=0.0):
    """model: PCALBSGarmentUseSegEncoderSeg; batch: the loader's keys skin_garment reads plus 'smpl_root_joints_torch' (nbatch,T,3);
    coeff_or_verts (nbatch, pca_dim) or (nbatch, Vg, 3); points (nbatch*T, P, 3); weights (nbatch*T, P) >= 0 or None; garment_faces (nf, 3) -> dict:
      data   fit.point_mesh_distance(points, verts, garment_faces, weights, trunc).loss on verts = posed garment + root joint (the root-offset
             convention of fit.scan_fit_loss: the clouds carry the offset, the posed garment does not)
      prior  coeff_prior * mean coeff^2   (coefficients only; 0 for vertices)
      total  their sum
    plus 'rms' (nbatch*T) and 'inliers' (nbatch*T) int32 of the data term, detached, and 'posed' (nbatch,T,Vg,3).  total.backward() fills .grad of
    coeff_or_verts (and of `points`, if it requires grad)."""
    _, posed = _posed_garment(model, body_model, batch, coeff_or_verts)
    nbatch, T, Vg = posed.shape[:3]
    root = batch["smpl_root_joints_torch"].to(posed.device).reshape(nbatch * T, 1, 3)
    verts = posed.reshape(nbatch * T, Vg, 3) + root
    f = fit.point_mesh_distance(points, verts, garment_faces, weights, trunc)
    prior = coeff_prior * (coeff_or_verts ** 2).mean() if coeff_or_verts.dim() == 2 else f.loss * 0
    return {"data": f.loss, "prior": prior, "total": f.loss + prior, "rms": f.rms, "inliers": f.inliers, "posed": posed}


def scan_garment_fit_loss(model, body_model, inputs, coeff_or_verts, garment_faces, garment_label, trunc=0.05, coeff_prior=0.0):
    """garment_fit_loss on a batch in the loader's form: points = inputs['pcd_torch'] (nbatch,T,N,3), weights = (inputs['pcd_label_torch'] ==
    garment_label) (the loader's label_dict[name] - 1, as scan.scan_batch writes it); `inputs` also holds the keys of `batch` above.
    Returns garment_fit_loss's dict with 'rms' and 'inliers' as (nbatch,T)."""
    pcd, lab = inputs["pcd_torch"], inputs["pcd_label_torch"]
    if not (torch.is_tensor(pcd) and pcd.dim() == 4 and pcd.shape[-1] == 3):
        raise ValueError("scan_garment_fit_loss: inputs['pcd_torch'] must be (nbatch, T, N, 3)")
    nbatch, T, N = (int(x) for x in pcd.shape[:3])
    if not (torch.is_tensor(lab) and lab.numel() == nbatch * T * N):
        raise ValueError("scan_garment_fit_loss: inputs['pcd_label_torch'] (nbatch, T, N, 1) expected")
    if not (pcd.is_cuda and pcd.dtype == torch.float32):
        raise TypeError("scan_garment_fit_loss: inputs['pcd_torch'] must be a float32 HIP tensor (no CPU fallback)")
    weights = (lab.reshape(nbatch * T, N) == int(garment_label)).to(torch.float32)
    out = garment_fit_loss(model, body_model, inputs, coeff_or_verts, pcd.reshape(nbatch * T, N, 3), weights, garment_faces, trunc, coeff_prior)
    out["rms"], out["inliers"] = out["rms"].view(nbatch, T), out["inliers"].view(nbatch, T)
    return out


def fit_garment_to_scan(model, body_model, batch, coeff_or_verts0, points, weights, garment_faces, steps, lr, trunc=0.05, coeff_prior=0.0):
    """`steps` steps of torch.optim.Adam(lr) on a copy of coeff_or_verts0, minimising garment_fit_loss(...)['total']: a plain loop, no line search,
    no staged schedule, nothing read back to the host.  Returns (fitted tensor (detached), losses): the device tensor of the steps + 1 totals --
    before every step, and after the last."""
    x = coeff_or_verts0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=lr)
    losses = torch.zeros(int(steps) + 1, dtype=torch.float32, device=points.device)
    for i in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        total = garment_fit_loss(model, body_model, batch, x, points, weights, garment_faces, trunc, coeff_prior)["total"]
        total.backward()
        losses[i] = total.detach()
        opt.step()
    with torch.no_grad():
        losses[int(steps)] = garment_fit_loss(model, body_model, batch, x, points, weights, garment_faces, trunc, coeff_prior)["total"]
    return x.detach(), losses


_label_cache = {}


def _joined_face_labels(faces, nfb, garment_label, device):
    """The labelling of scan.scan_batch for the joined mesh: body faces 0, garment faces `garment_label`; (nf) int32 on `device`, once per mesh."""
    def build():
        assert not torch.cuda.is_current_stream_capturing(), "garment_fit: build the face labels before the capture (call once eagerly)"
        host = np.zeros(len(faces), np.int32)
        host[nfb:] = int(garment_label)
        return torch.from_numpy(host).to(device)
    return _cache.by_identity(_label_cache, 8, (faces,), (int(nfb), int(garment_label), str(device)), build)


def depth_garment_fit_loss(model, body_model, batch, coeff_or_verts, depth_obs, labels_obs, cameras, garment_faces, garment_label, weights=None, trunc=0.05,
                           grazing=0.1, coeff_prior=0.0):
    """garment_fit_loss for data that comes as depth images: depth_obs (K,nbatch*T,h,w) and labels_obs (K,nbatch*T,h,w) int32 of the K `cameras`
    (what depth_fit.sensor_depth gives with scan.scan_batch's labelling: body 0, garment `garment_label`, background -1), weights or None.
    The mesh is the body batch['smpl_vertices_torch'] (nbatch,T,Vb,3) -- a constant -- joined with the posed garment + root joint
    (render._joined_faces), so the body occludes the garment as it does for the sensor, and a garment ray pairs only with a garment face.
    data = depth_fit.depth_mesh_distance(...).loss over the rays of BOTH labels (the body's rays carry no gradient: its vertices are constants;
    pass weights = (labels_obs == garment_label) to leave them out of W); the gradient reaches the garment vertices through the torch.cat and goes
    on through the skinning adjoint.  prior, total, rms, inliers, posed: garment_fit_loss's."""
    _, posed = _posed_garment(model, body_model, batch, coeff_or_verts)
    nbatch, T, Vg = posed.shape[:3]
    body = batch["smpl_vertices_torch"].to(posed.device)
    if not (body.dim() == 4 and tuple(body.shape[:2]) == (nbatch, T) and body.shape[-1] == 3):
        raise ValueError("depth_garment_fit_loss: batch['smpl_vertices_torch'] must be (nbatch, T, Vb, 3)")
    Vb = int(body.shape[2])
    root = batch["smpl_root_joints_torch"].to(posed.device).reshape(nbatch * T, 1, 3)
    verts = torch.cat([body.reshape(nbatch * T, Vb, 3).detach(), posed.reshape(nbatch * T, Vg, 3) + root], 1)
    faces = render._joined_faces(body_model.faces, garment_faces, Vb)
    face_labels = _joined_face_labels(faces, int(np.asarray(body_model.faces).shape[0]), garment_label, posed.device)
    f = depth_fit.depth_mesh_distance(depth_obs, verts, faces, cameras, weights, trunc, grazing, labels_obs, face_labels)
    prior = coeff_prior * (coeff_or_verts ** 2).mean() if coeff_or_verts.dim() == 2 else f.loss * 0
    return {"data": f.loss, "prior": prior, "total": f.loss + prior, "rms": f.rms, "inliers": f.inliers, "posed": posed}


def fit_garment_to_depth(model, body_model, batch, coeff_or_verts0, depth_obs, labels_obs, cameras, garment_faces, garment_label, steps, lr, weights=None,
                         trunc=0.05, grazing=0.1, coeff_prior=0.0):
    """fit_garment_to_scan's plain Adam loop on depth_garment_fit_loss(...)['total']: the joined mesh is rasterized anew at every step.  Returns
    (fitted tensor (detached), losses) as fit_garment_to_scan does."""
    x = coeff_or_verts0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=lr)
    losses = torch.zeros(int(steps) + 1, dtype=torch.float32, device=depth_obs.device)
    args = (depth_obs, labels_obs, cameras, garment_faces, garment_label, weights, trunc, grazing, coeff_prior)
    for i in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        total = depth_garment_fit_loss(model, body_model, batch, x, *args)["total"]
        total.backward()
        losses[i] = total.detach()
        opt.step()
    with torch.no_grad():
        losses[int(steps)] = depth_garment_fit_loss(model, body_model, batch, x, *args)["total"]
    return x.detach(), losses
