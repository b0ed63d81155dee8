"""Fit a mesh to a scan on HIP: the distance of every scan point to the surface of a predicted mesh, truncated, weighted and summed into one
loss, and that loss's gradient to the mesh vertices (and to the points) -- the data term of scan registration, and the one supervision there is
on captured data, where no ground-truth mesh exists.  scan.py produces exactly such inputs (`pcd_torch` / `pcd_label_torch`).

One direction only, points -> surface: a one-sided scan says nothing about the surface it did not see.  The nearest face of every point
comes from postprocess's exact search (g4d_mesh_nearest_f32) and is held fixed in the backward, as in any such loss; csrc/fit/fit.hip
(libg4d_fit.so) recomputes the closest point on that face as barycentric weights -- the search's own routine, the same bits --, reduces, groups
the inliers by face with an LDS sort and gathers the vertex gradient.  include/g4d_fit.h is the contract, tests/fit_twin.py the numpy
restatement.  fp32 on the current torch stream, no atomics, no host round trip: two runs give the same bits, and after one eager call (which
builds the per-topology tables on the host, cached by the identity of `faces`) the functional calls can be captured in a hipGraph.  There is no
fallback: without the library, or on a CPU tensor, the calls raise.

Domain of the backward: P <= 32768 points per frame and nf <= 131072 faces (a sort key holds both); beyond it the calls raise before any launch."""
import collections
import math

import numpy as np
import torch

from . import _cache
from . import _lib
from . import mesh_tables
from . import postprocess

Terms = collections.namedtuple("Terms", "bary resid dist2 inlier sums count total")
Fit = collections.namedtuple("Fit", "loss per_frame rms inliers nearest")


def _f32(name, t, last=3):
    if not (torch.is_tensor(t) and t.dim() == 3 and t.shape[-1] == last):
        raise ValueError(f"{name} must be (F, n, {last})")
    if not (t.is_cuda and t.dtype == torch.float32):
        raise TypeError(f"{name}: a float32 HIP tensor of shape (F, n, {last}) expected (no CPU fallback)")
    return t.contiguous()


def _weights(name, w, F_, P):
    if w is None:
        return None
    if not (torch.is_tensor(w) and w.numel() == F_ * P and tuple(w.shape[:2]) == (F_, P)):
        raise ValueError(f"{name}: weights must be (F, P) = ({F_}, {P})")
    if not (w.is_cuda and w.dtype == torch.float32):
        raise TypeError(f"{name}: weights: a float32 HIP tensor expected (no CPU fallback)")
    return w.reshape(F_, P).contiguous()


def _tau2(trunc):
    if trunc is None:
        return math.inf
    t = np.float32(trunc)
    return float(t * t)      # the square of the fp32 distance, rounded once


_corner_cache = {}


def vertex_corner_table(faces, num_verts, device):
    """The vertex -> (face * 3 + corner) CSR of `faces` as int32 tensors (rowptr (V + 1), corners (3 nf)), entries ascending per vertex
    (mesh_tables.vertex_corners), built once per `faces` object: host work, so call once before any hipGraph capture."""
    def build():
        assert not torch.cuda.is_current_stream_capturing(), "fit: build the corner table before the capture (call once eagerly)"
        f = np.ascontiguousarray((faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64)).reshape(-1, 3)
        if len(f) and (f.min() < 0 or f.max() >= num_verts):
            raise ValueError(f"fit: face indices must lie in [0, {num_verts})")
        rowptr, corners = mesh_tables.vertex_corners(f, num_verts)
        return mesh_tables.to_device(rowptr, np.int32, device), mesh_tables.to_device(corners, np.int32, device), int(len(f))

    return _cache.by_identity(_corner_cache, 16, (faces,), (int(num_verts), str(device)), build)


def point_face_terms(points, verts, faces_dev, face, weights=None, tau2=math.inf):
    """g4d_fit_point_face_f32: points (F,P,3), verts (F,V,3), faces_dev (nf,3) int32 HIP tensor in the order `face` (F,P) int32 indexes, weights
    (F,P) or None, tau2 the SQUARED truncation distance -> Terms(bary (F,P,3), resid (F,P,3), dist2 (F,P), inlier (F,P) int32, sums (F,3) =
    (sum w d2 over inliers, sum w over inliers, sum w over all points), count (F) int32, total (2) = (W, loss))."""
    F_, P, _ = points.shape
    V, nf, dev = int(verts.shape[1]), int(faces_dev.shape[0]), points.device
    out = Terms(torch.zeros((F_, P, 3), dtype=torch.float32, device=dev), torch.zeros((F_, P, 3), dtype=torch.float32, device=dev),
                torch.zeros((F_, P), dtype=torch.float32, device=dev), torch.zeros((F_, P), dtype=torch.int32, device=dev),
                torch.zeros((F_, 3), dtype=torch.float32, device=dev), torch.zeros((F_,), dtype=torch.int32, device=dev),
                torch.zeros((2,), dtype=torch.float32, device=dev))
    _lib.fit_lib()
    _lib.call("g4d_fit_point_face_f32", F_, P, V, nf, points.data_ptr(), verts.data_ptr(), faces_dev.data_ptr(), face.data_ptr(),
              weights.data_ptr() if weights is not None else None, float(tau2), out.bary.data_ptr(), out.resid.data_ptr(), out.dist2.data_ptr(),
              out.inlier.data_ptr(), out.sums.data_ptr(), out.count.data_ptr(), out.total.data_ptr(), _lib.stream_ptr())
    return out


def group_by_face(face, inlier, nf):
    """g4d_fit_group_f32: face, inlier (F,P) int32 -> keys (F,P) int32 holding the uint32 bits face << 15 | index of every frame's inliers in
    ascending order (by face, then by point index), 0xFFFFFFFF (-1) after them."""
    F_, P = face.shape
    keys = torch.full((F_, P), -1, dtype=torch.int32, device=face.device)
    _lib.fit_lib()
    _lib.call("g4d_fit_group_f32", F_, P, int(nf), face.data_ptr(), inlier.data_ptr(), keys.data_ptr(), _lib.stream_ptr())
    return keys


def vertex_gradient(terms, keys, grad_out, corner_table, num_verts, weights=None, want_points=False):
    """g4d_fit_vertex_grad_f32: the gradient of grad_out * loss to the vertices (F,V,3) and, if asked for, to the points (F,P,3) (else None).
    grad_out: a float32 HIP tensor of one element -- read on the device, nothing comes back to the host.  corner_table: vertex_corner_table()."""
    F_, P, _ = terms.bary.shape
    rowptr, corners, nf = corner_table
    dev = terms.bary.device
    gv = torch.zeros((F_, int(num_verts), 3), dtype=torch.float32, device=dev)
    gp = torch.zeros((F_, P, 3), dtype=torch.float32, device=dev) if want_points else None
    _lib.fit_lib()
    _lib.call("g4d_fit_vertex_grad_f32", F_, P, int(num_verts), nf, terms.bary.data_ptr(), terms.resid.data_ptr(), terms.inlier.data_ptr(),
              weights.data_ptr() if weights is not None else None, keys.data_ptr(), terms.count.data_ptr(), terms.total.data_ptr(), grad_out.data_ptr(),
              rowptr.data_ptr(), corners.data_ptr(), gv.data_ptr(), gp.data_ptr() if gp is not None else None, _lib.stream_ptr())
    return gv, gp


class _PointMeshLoss(torch.autograd.Function):
    """loss = total[1] of point_face_terms; backward = group_by_face + vertex_gradient with the nearest faces of the forward."""

    @staticmethod
    def forward(ctx, points, verts, weights, face, faces_dev, corner_table, tau2):
        terms = point_face_terms(points, verts, faces_dev, face, weights, tau2)
        ctx.terms, ctx.face, ctx.weights, ctx.table, ctx.num_verts = terms, face, weights, corner_table, int(verts.shape[1])
        ctx.mark_non_differentiable(terms.sums, terms.count)
        return terms.total[1].clone(), terms.sums, terms.count

    @staticmethod
    def backward(ctx, grad_loss, _sums, _count):
        need_p, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        keys = group_by_face(ctx.face, ctx.terms.inlier, ctx.table[2])
        gv, gp = vertex_gradient(ctx.terms, keys, g, ctx.table, ctx.num_verts if need_v else 0, ctx.weights, want_points=need_p)
        return gp, (gv if need_v else None), None, None, None, None, None


def point_mesh_distance(points, verts, faces, weights=None, trunc=None, template=None):
    """points (F,P,3), verts (F,V,3) float32 HIP tensors, faces (nf,3) shared by the frames, weights (F,P) >= 0 or None (all 1), trunc: the
    truncation DISTANCE (None: none) -> Fit(loss, per_frame (F,3), rms (F), inliers (F) int32, nearest).

    nearest = postprocess.nearest_on_mesh(points, verts, faces, template): face i of a point is held fixed from here on.  A point is an inlier
    iff its weight is > 0, it has a face, and dist2 < trunc^2 (strict; a NaN distance never is).  With W = the sum of ALL weights,
    loss = (sum over inliers of w dist2) / W -- 0, with zero gradients, when W == 0.  per_frame[f] = (sum w dist2, sum w, number) over the frame's
    inliers; rms[f] = sqrt of the first over the second (0 for a frame without inliers): the weighted RMS distance.
    loss is the output of one autograd.Function: loss.backward() fills .grad of `verts` and / or `points`, whichever requires grad, by
    g4d_fit_group_f32 + g4d_fit_vertex_grad_f32 (P <= 32768, nf <= 131072, else G4DError before any launch); everything else is detached.
    Raises TypeError for anything but float32 HIP tensors ("... (no CPU fallback)"), ValueError for a wrong shape."""
    pts, v = _f32("point_mesh_distance: points", points), _f32("point_mesh_distance: verts", verts)
    F_, P, _ = pts.shape
    if v.shape[0] != F_:
        raise ValueError(f"point_mesh_distance: {F_} frames of points, {v.shape[0]} frames of mesh")
    w = _weights("point_mesh_distance", weights, F_, P)
    with torch.no_grad():
        mesh = postprocess._SearchMesh(v.detach(), faces, template)
        near = mesh.nearest(pts.detach())
    table = vertex_corner_table(faces, int(v.shape[1]), v.device)
    loss, sums, count = _PointMeshLoss.apply(pts, v, w, near.face, mesh.topo["faces"], table, _tau2(trunc))
    s, win = sums[:, 0], sums[:, 1]
    rms = torch.where(win > 0, torch.sqrt(s / torch.where(win > 0, win, torch.ones_like(win))), torch.zeros_like(win))
    return Fit(loss, torch.stack([s, win, count.to(torch.float32)], 1), rms, count, near)


def scan_fit_loss(output_dict, inputs, garment_faces, garment_label, trunc=0.05, round=-1):
    """The distance of the garment-labelled points of the input cloud to the garment the model predicted from it.
    points = inputs['pcd_torch'] (nbatch,T,N,3), weights = (inputs['pcd_label_torch'] == garment_label) (the loader's label_dict[name] - 1, as
    scan.scan_batch writes it), verts = output_dict['iter_regressed_lbs_garment_v'][round] (nbatch*T,Vg,3) PLUS inputs['smpl_root_joints_torch']
    (nbatch,T,3): the clouds carry the root offset, the predictions do not (scan.scan_batch adds the same offset before it scans).
    Returns {'scan_fit_loss': scalar, 'scan_fit_rms_list': (nbatch,T), 'scan_fit_inliers': (nbatch,T) int32}.  Under tuning.refine_autograd the
    loss's backward reaches the refinement head's parameters and nothing of the encoder."""
    pcd, lab, root = inputs["pcd_torch"], inputs["pcd_label_torch"], inputs["smpl_root_joints_torch"]
    if not (torch.is_tensor(pcd) and pcd.dim() == 4 and pcd.shape[-1] == 3):
        raise ValueError("scan_fit_loss: inputs['pcd_torch'] must be (nbatch, T, N, 3)")
    nbatch, T, N = (int(x) for x in pcd.shape[:3])
    if not (torch.is_tensor(lab) and lab.numel() == nbatch * T * N and torch.is_tensor(root) and root.numel() == nbatch * T * 3):
        raise ValueError("scan_fit_loss: inputs['pcd_label_torch'] (nbatch, T, N, 1) and inputs['smpl_root_joints_torch'] (nbatch, T, 3) expected")
    g = output_dict["iter_regressed_lbs_garment_v"][round]
    for name, t in (("inputs['pcd_torch']", pcd), ("inputs['smpl_root_joints_torch']", root), ("the predicted garment", g)):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise TypeError(f"scan_fit_loss: {name} must be a float32 HIP tensor (no CPU fallback)")
    verts = g.reshape(nbatch * T, -1, 3) + root.reshape(nbatch * T, 1, 3)
    weights = (lab.reshape(nbatch * T, N) == int(garment_label)).to(torch.float32)
    fit = point_mesh_distance(pcd.reshape(nbatch * T, N, 3), verts, garment_faces, weights, trunc)
    return {"scan_fit_loss": fit.loss, "scan_fit_rms_list": fit.rms.view(nbatch, T), "scan_fit_inliers": fit.inliers.view(nbatch, T)}
