"""Fit a mesh to depth images on HIP: a second data term next to fit.point_mesh_distance, for data that comes as one depth per ray of a known
camera instead of an unordered cloud.  Registration pipelines built on depth sensors (KinectFusion, DynamicFusion and their descendants) pair each
observed ray with the face of the current estimate that ray sees -- projective data association -- and penalise the difference in depth along the
ray: no nearest-face search.  Here the association comes from the exact-coverage rasterizer (render.py, once per camera, under no_grad);
csrc/depth/depth_fit.hip (libg4d_depth.so) intersects each ray with its face's plane from the un-snapped camera-space vertices, truncates,
weights and sums the squared residuals into one loss, and gathers the gradient to the mesh vertices with the visible face held fixed.
include/g4d_depth.h is the contract, tests/depth_fit_twin.py the numpy restatement.

What it does not do: an observed miss over a predicted hit (free space, silhouette) carries no gradient; nothing is differentiated to the camera
or through the rasterizer.  fp32 on the current torch stream, no atomics, no host round trip: two runs give the same bits, and after one eager
call (which builds the corner table and the host copy of `faces`, cached by the identity of `faces`) the calls can be captured in a hipGraph.
There is no fallback: without the library, or on a CPU tensor, the calls raise."""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import fit
from . import render

SensorDepth = collections.namedtuple("SensorDepth", "depth labels face_id")
DepthTerms = collections.namedtuple("DepthTerms", "sums count total resid")
DepthFit = collections.namedtuple("DepthFit", "loss per_frame rms inliers face_id")
Views = collections.namedtuple("Views", "px py invz cam face_id depth cams_host")
MAX_CAMS = 8      # G4D_DEPTH_MAX_CAMS (tests/test_depth_fit_cpu.py holds the two together)
MAX_SIDE = 4096   # G4D_DEPTH_MAX_SIDE


def chunk():
    """Samples per workgroup of the forward (g4d_depth_chunk)."""
    return int(_lib.depth_lib()[0].g4d_depth_chunk())


def camera_constants(cameras):
    """(K,10) float32 host array: per camera the rows of the look-at basis as g4d_render_project_f32 rounds them to fp32, then its fp32 1 / tan."""
    out = np.zeros((len(cameras), 10), np.float32)
    for c, cam in enumerate(cameras):
        out[c, :9] = render.camera_rotation(cam).astype(np.float32).reshape(9)
        out[c, 9] = np.float32(1.0 / math.tan(float(np.float32(cam.half_angle)) * (math.pi / 180.0)))
    return out


def _check_cameras(who, cameras, image_size):
    cameras = list(cameras) if cameras is not None else None
    if cameras is None or not 1 <= len(cameras) <= MAX_CAMS:
        raise ValueError(f"{who}: 1 to {MAX_CAMS} cameras ({0 if cameras is None else len(cameras)} given)")
    w, h = render._size(image_size)
    if not (0 <= w <= MAX_SIDE and 0 <= h <= MAX_SIDE):
        raise ValueError(f"{who}: a sensor of at most {MAX_SIDE} x {MAX_SIDE} rays ({w} x {h} given)")
    return cameras, w, h


def _verts_shape(who, verts):
    if not (torch.is_tensor(verts) and verts.dim() == 3 and verts.shape[-1] == 3):
        raise ValueError(f"{who}: verts must be (F, V, 3)")


def _verts(who, verts):
    _verts_shape(who, verts)
    if not (verts.is_cuda and verts.dtype == torch.float32):
        raise TypeError(f"{who}: verts: a float32 HIP tensor of shape (F, V, 3) expected (no CPU fallback)")
    return verts.contiguous()


def _image(who, name, t, shape, dtype):
    if t is None:
        return None
    if not (torch.is_tensor(t) and tuple(t.shape) == shape):
        raise ValueError(f"{who}: {name} must be (K, F, h, w) = {shape}")
    if not (t.is_cuda and t.dtype == dtype):
        raise TypeError(f"{who}: {name}: a {str(dtype).replace('torch.', '')} HIP tensor expected (no CPU fallback)")
    return t.contiguous()


def _face_labels(who, face_labels, nf):
    if face_labels is not None and not (torch.is_tensor(face_labels) and face_labels.is_cuda and face_labels.dtype == torch.int32
                                        and tuple(face_labels.shape) == (nf,)):
        raise TypeError(f"{who}: face_labels must be an int32 HIP tensor of shape ({nf},) (no CPU fallback)")
    return face_labels.contiguous() if face_labels is not None else None


def views(verts, faces, cameras, w, h):
    """What every camera sees of verts (F,V,3): per camera render.project at ss = 1 and render.rasterize(want_image=False), stacked camera-major ->
    Views(px, py (K,F,V) int32, invz (K,F,V), cam (K,F,V,3), face_id (K,F,h,w) int32, depth (K,F,h,w), cams_host (K,10))."""
    with torch.no_grad():
        proj = [render.project(verts, cam, (w, h), 1) for cam in cameras]
        ras = [render.rasterize(p.px, p.py, p.invz, faces, (w, h), 1, want_image=False) for p in proj]
        px, py, invz, cam = (torch.stack([getattr(p, name) for p in proj]) for name in ("px", "py", "invz", "cam"))
        return Views(px, py, invz, cam, torch.stack([r.face_id for r in ras]), torch.stack([r.depth for r in ras]), camera_constants(cameras))


def sensor_depth(verts, faces, cameras, image_size=256, face_labels=None):
    """What the virtual sensor of scan.py sees, as images instead of a resampled cloud: verts (F,V,3) float32 HIP tensor in world space, faces
    (nf,3) shared by the frames, cameras: 1 to 8 render.Camera, image_size: the sensor's rays, w or (w, h) ->
    SensorDepth(depth (K,F,h,w) = the rasterizer's camera-space z of the visible surface, +inf on the background; labels (K,F,h,w) int32 =
    face_labels[face_id], -1 on the background, or None without face_labels ((nf) int32 HIP tensor); face_id (K,F,h,w) int32)."""
    who = "sensor_depth"
    _verts_shape(who, verts)
    cameras, w, h = _check_cameras(who, cameras, image_size)
    v = _verts(who, verts)
    nf = int(render._faces(faces, v.device)[1].shape[0])
    face_labels = _face_labels(who, face_labels, nf)
    s = views(v.detach(), faces, cameras, w, h)
    labels = None
    if face_labels is not None:
        seen = s.face_id >= 0
        labels = torch.where(seen, face_labels[s.face_id.clamp_min(0).long()] if nf else torch.zeros_like(s.face_id), torch.full_like(s.face_id, -1))
    return SensorDepth(s.depth, labels, s.face_id)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _host(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def depth_terms(s, faces_dev, depth_obs, weights=None, labels_obs=None, face_labels=None, trunc=math.inf, grazing=0.1, want_resid=False):
    """g4d_depth_fit_terms_f32 on Views `s`: -> DepthTerms(sums (F,3) = (sum w r^2 over inliers, sum w over inliers, sum w over observed rays),
    count (F) int32, total (2) = (W, loss), resid (K,F,h,w) with NaN where there is no inlier, or None)."""
    K, F_, V = s.px.shape
    h, w = int(s.face_id.shape[2]), int(s.face_id.shape[3])
    nf, dev = int(faces_dev.shape[0]), s.px.device
    L, _, _ = _lib.depth_lib()
    ws = _lib.workspace(int(L.g4d_depth_ws_bytes(F_, K, w, h)), dev)
    out = DepthTerms(torch.zeros((F_, 3), dtype=torch.float32, device=dev), torch.zeros((F_,), dtype=torch.int32, device=dev),
                     torch.zeros((2,), dtype=torch.float32, device=dev),
                     torch.full((K, F_, h, w), math.nan, dtype=torch.float32, device=dev) if want_resid else None)
    _lib.call("g4d_depth_fit_terms_f32", F_, K, V, nf, w, h, _ptr(s.cam), _ptr(faces_dev), s.face_id.data_ptr(), depth_obs.data_ptr(), _ptr(weights),
              _ptr(labels_obs), _ptr(face_labels), _host(s.cams_host), float(trunc), float(grazing), ws.data_ptr(), ws.numel(), out.sums.data_ptr(),
              out.count.data_ptr(), out.total.data_ptr(), _ptr(out.resid), _lib.stream_ptr())
    return out


def depth_vertex_gradient(s, faces_dev, depth_obs, total, grad_out, corner_table, weights=None, labels_obs=None, face_labels=None, trunc=math.inf,
                          grazing=0.1):
    """g4d_depth_fit_vertex_grad_f32: the gradient of grad_out * loss to the vertices (F,V,3).  grad_out: a float32 HIP tensor of one element --
    read on the device, nothing comes back to the host.  corner_table: fit.vertex_corner_table()."""
    K, F_, V = s.px.shape
    h, w = int(s.face_id.shape[2]), int(s.face_id.shape[3])
    rowptr, corners, nf = corner_table
    gv = torch.zeros((F_, V, 3), dtype=torch.float32, device=s.px.device)
    _lib.depth_lib()
    _lib.call("g4d_depth_fit_vertex_grad_f32", F_, K, V, nf, w, h, s.px.data_ptr(), s.py.data_ptr(), s.invz.data_ptr(), s.cam.data_ptr(),
              _ptr(faces_dev), s.face_id.data_ptr(), depth_obs.data_ptr(), _ptr(weights), _ptr(labels_obs), _ptr(face_labels), _host(s.cams_host),
              float(trunc), float(grazing), total.data_ptr(), grad_out.data_ptr(), rowptr.data_ptr(), _ptr(corners) if nf else None, gv.data_ptr(),
              _lib.stream_ptr())
    return gv


class _DepthMeshLoss(torch.autograd.Function):
    """loss = total[1] of depth_terms; backward = depth_vertex_gradient with the association of the forward."""

    @staticmethod
    def forward(ctx, verts, s, faces_dev, depth_obs, weights, labels_obs, face_labels, corner_table, trunc, grazing):
        terms = depth_terms(s, faces_dev, depth_obs, weights, labels_obs, face_labels, trunc, grazing)
        ctx.args = (s, faces_dev, depth_obs, terms.total, corner_table, weights, labels_obs, face_labels, trunc, grazing)
        ctx.mark_non_differentiable(terms.sums, terms.count)
        return terms.total[1].clone(), terms.sums, terms.count

    @staticmethod
    def backward(ctx, grad_loss, _sums, _count):
        s, faces_dev, depth_obs, total, table, weights, labels_obs, face_labels, trunc, grazing = ctx.args
        g = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        gv = depth_vertex_gradient(s, faces_dev, depth_obs, total, g, table, weights, labels_obs, face_labels, trunc, grazing)
        return (gv,) + (None,) * 9


def depth_mesh_distance(depth_obs, verts, faces, cameras, weights=None, trunc=None, grazing=0.1, labels=None, face_labels=None, image_size=None):
    """depth_obs (K,F,h,w) float32 HIP tensor: the observed depth images of K cameras (camera-space z; anything not finite or <= 0 is no
    observation), verts (F,V,3) float32 HIP tensor, faces (nf,3) shared by the frames, cameras: the K render.Camera, weights (K,F,h,w) >= 0 or
    None (all 1), trunc: the truncation of |residual| (None: none), grazing: the smallest |cosine| between ray and face normal still used (0.1,
    about 84 degrees: an interface default, not a measured quantity), labels (K,F,h,w) int32 with face_labels (nf) int32: a ray pairs only with a
    face of its own label (both or neither), image_size: w or (w, h), checked against depth_obs when given
    -> DepthFit(loss, per_frame (F,3), rms (F), inliers (F) int32, face_id (K,F,h,w)).

    verts.detach() is projected and rasterized under no_grad (render.project + render.rasterize at ss = 1 per camera): face_id is the face every
    ray sees, held fixed from here on.  A ray is an inlier iff its weight is > 0, it is observed, sees a face (of its label), that face is not
    grazing and |z - depth_obs| < trunc with z the depth at which the ray meets the face's plane (include/g4d_depth.h).  With W = the sum of the
    weights of ALL observed rays, loss = (sum over inliers of w (z - depth_obs)^2) / W -- 0, with zero gradients, when W == 0.  per_frame[f] =
    (sum w r^2, sum w, number) over the frame's inliers; rms[f] = sqrt of the first over the second (0 for a frame without inliers).
    loss is the output of one autograd.Function: loss.backward() fills .grad of `verts` by g4d_depth_fit_vertex_grad_f32; depth_obs is data and
    gets no gradient.  Raises TypeError for anything but HIP tensors of the documented dtype ("... (no CPU fallback)"), ValueError for a wrong
    shape, more than 8 cameras or a sensor beyond 4096 x 4096 -- before any launch."""
    who = "depth_mesh_distance"
    if not (torch.is_tensor(depth_obs) and depth_obs.dim() == 4):
        raise ValueError(f"{who}: depth_obs must be (K, F, h, w)")
    _verts_shape(who, verts)
    K, F_, h, w = (int(x) for x in depth_obs.shape)
    cameras, w, h = _check_cameras(who, cameras, (w, h))
    if len(cameras) != K or verts.shape[0] != F_:
        raise ValueError(f"{who}: depth_obs is (K, F, h, w) = {tuple(depth_obs.shape)}: {len(cameras)} cameras and {verts.shape[0]} frames of mesh given")
    if image_size is not None and render._size(image_size) != (w, h):
        raise ValueError(f"{who}: image_size {render._size(image_size)} but depth_obs holds {w} x {h} rays")
    if (labels is None) != (face_labels is None):
        raise ValueError(f"{who}: labels and face_labels go together")
    v = _verts(who, verts)
    shape = (K, F_, h, w)
    d = _image(who, "depth_obs", depth_obs, shape, torch.float32)
    wt = _image(who, "weights", weights, shape, torch.float32)
    lab = _image(who, "labels", labels, shape, torch.int32)
    f_dev, f_host = render._faces(faces, v.device)
    nf = int(f_host.shape[0])
    fl = _face_labels(who, face_labels, nf)
    if nf == 0:
        lab = fl = None      # nothing associates either way
    table = fit.vertex_corner_table(faces, int(v.shape[1]), v.device)
    s = views(v.detach(), faces, cameras, w, h)
    loss, sums, count = _DepthMeshLoss.apply(v, s, f_dev, d, wt, lab, fl, table, math.inf if trunc is None else float(np.float32(trunc)), float(grazing))
    sr, win = sums[:, 0], sums[:, 1]
    rms = torch.where(win > 0, torch.sqrt(sr / torch.where(win > 0, win, torch.ones_like(win))), torch.zeros_like(win))
    return DepthFit(loss, torch.stack([sr, win, count.to(torch.float32)], 1), rms, count, s.face_id)
