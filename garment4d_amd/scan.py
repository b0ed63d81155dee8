"""Virtual depth-sensor scans on HIP: meshes seen from one or several cameras become fixed-size, labelled world-space point clouds in the
form of the data loader's `inputs['pcd_torch']` / `inputs['pcd_label_torch']` (utils/dataloader.py:215-230, 279).  Where the loader takes
every body vertex and half of the garment's -- a full, view-independent vertex set -- a scan holds what a depth camera or LiDAR delivers: the
surface the cameras see, one-sided and self-occluded, as dense as the sensor's rays fall on it, each point labelled body or garment.

Per camera the rasterizer (render.py) gives the visible face of every ray; csrc/scan/scan.hip (libg4d_scan.so) ranks the hits of all cameras,
selects exactly `n_points` of them per frame (stratified over the hits in scan order when there are enough, repeating them when there are
not) and unprojects each selected hit exactly, perspective-correct from its face's world-space vertices.  include/g4d_scan.h is the contract,
tests/scan_twin.py the numpy restatement.  Three launches, no atomics, no host round trip and no allocation inside the call, bit-reproducible:
after one eager call (which copies `faces` to the host once per faces object, see render._faces) a call can be captured in a hipGraph.
There is no fallback: without the library, or on a CPU tensor, the calls raise.

Point order is SCAN order -- camera, then row, then column.  The loader shuffles its cloud (`random_sample_pcd`); this does not: a caller who
wants a shuffle applies `torch.randperm` to the point axis (of `points` and `labels` alike)."""
import collections

import numpy as np
import torch

from . import _cache
from . import _lib
from . import render

Scan = collections.namedtuple("Scan", "points labels face sample count")
MAX_CAMS = 8   # G4D_SCAN_MAX_CAMS (tests/test_scan_cpu.py holds the two together)


def chunk():
    """Samples per workgroup of the counting and the selecting launch (g4d_scan_chunk)."""
    return int(_lib.scan_lib()[0].g4d_scan_chunk())


def ring_cameras(k, distance=1.5, elevation=0.0, start=45.0):
    """k look-at cameras (render.look_at_camera) around the origin at azimuths start + 360 i / k degrees, i = 0 .. k - 1."""
    return [render.look_at_camera(distance, elevation, start + 360.0 * i / k) for i in range(int(k))]


def scan_meshes(verts, faces, cameras=None, image_size=256, n_points=8192, face_labels=None, seed=0, noise_sigma=0.0, generator=None):
    """verts (F,V,3) float32 HIP tensor in world space, faces (nf,3) shared by the frames, cameras: 1 to 8 render.Camera (default: the one of
    render_meshes, distance 1.5, azimuth 45), image_size: the sensor's rays, w or (w, h), one sample per ray ->
    Scan(points (F,N,3), labels (F,N) int32, face (F,N) int32, sample (F,N) int32, count (F) int32), N = n_points.
    Per camera g4d_render_project_f32 and g4d_render_raster at ss = 1, then g4d_scan_points_f32 (include/g4d_scan.h): `count` is the number
    of rays of all cameras that hit the mesh; `points` are exactly N of the hits in scan order (camera, row, column; NOT shuffled) --
    stratified without replacement when count >= N, every hit floor or ceil(N / count) times when 0 < count < N; `face` is the face a
    point lies on, `sample` its ray (c h + i) w + j, so its camera is sample // (h w); labels = face_labels[face] (face_labels: (nf) int32
    HIP tensor), 0 without face_labels.  A frame no ray hits has points 0 and labels, face, sample -1.  Same seed, same bits.
    noise_sigma > 0 moves each point along its viewing ray (point - eye of its camera, normalised) by noise_sigma * randn (`generator`: the
    torch.Generator of the draw): plain torch, outside the contract, off by default.
    Raises TypeError for anything but HIP tensors of the documented dtype ("... HIP tensor ... (no CPU fallback)"), ValueError for a wrong
    shape ("scan_meshes: verts must be (F, V, 3)", "scan_meshes: 1 to 8 cameras")."""
    if not (torch.is_tensor(verts) and verts.dim() == 3 and verts.shape[-1] == 3):
        raise ValueError("scan_meshes: verts must be (F, V, 3)")
    cameras = list(cameras) if cameras is not None else ring_cameras(1)
    if not 1 <= len(cameras) <= MAX_CAMS:
        raise ValueError(f"scan_meshes: 1 to {MAX_CAMS} cameras ({len(cameras)} given)")
    v = render._f32("scan_meshes: verts", verts, (3,))
    L, _, _ = _lib.scan_lib()
    F_, V = int(v.shape[0]), int(v.shape[1])
    K, N, dev = len(cameras), int(n_points), v.device
    w, h = render._size(image_size)
    f_dev, f_host = render._faces(faces, dev)
    nf = int(f_host.shape[0])
    if face_labels is not None and not (torch.is_tensor(face_labels) and face_labels.is_cuda and face_labels.dtype == torch.int32
                                        and tuple(face_labels.shape) == (nf,)):
        raise TypeError(f"scan_meshes: face_labels must be an int32 HIP tensor of shape ({nf},) (no CPU fallback)")
    views = [render.project(v, cam, (w, h), 1) for cam in cameras]
    ids = torch.stack([render.rasterize(p.px, p.py, p.invz, faces, (w, h), 1, want_image=False).face_id for p in views])
    px, py, invz = (torch.stack([getattr(p, name) for p in views]) for name in ("px", "py", "invz"))
    ws = _lib.workspace(int(L.g4d_scan_ws_bytes(F_, K, w, h)), dev)
    out = Scan(torch.empty((F_, N, 3), dtype=torch.float32, device=dev), *(torch.empty((F_, N), dtype=torch.int32, device=dev) for _ in range(3)),
               torch.zeros((F_,), dtype=torch.int32, device=dev))
    _lib.call("g4d_scan_points_f32", F_, K, V, nf, w, h, px.data_ptr(), py.data_ptr(), invz.data_ptr(), ids.data_ptr(), v.data_ptr(), f_dev.data_ptr(),
              face_labels.contiguous().data_ptr() if face_labels is not None else None, N, int(seed) & 0xFFFFFFFF, ws.data_ptr(), ws.numel(),
              out.points.data_ptr(), out.labels.data_ptr(), out.face.data_ptr(), out.sample.data_ptr(), out.count.data_ptr(), _lib.stream_ptr())
    if noise_sigma > 0:
        eyes = torch.tensor([c.eye for c in cameras], dtype=torch.float32, device=dev)
        seen = (out.sample >= 0).unsqueeze(-1)
        ray = out.points - eyes[torch.div(out.sample.clamp_min(0), h * w, rounding_mode="floor").long()]
        ray = ray / ray.norm(dim=-1, keepdim=True).clamp_min(1e-20)
        step = float(noise_sigma) * torch.randn((F_, N, 1), dtype=torch.float32, device=dev, generator=generator)
        out = out._replace(points=torch.where(seen, out.points + ray * step, out.points))
    return out


_label_cache = {}


def scan_batch(inputs, body_model, garment_faces, garment_label, cameras=None, n_points=8192, seed=0, image_size=256):
    """A batch of the data loader, scanned: the body inputs['smpl_vertices_torch'] (nbatch,T,Vb,3) and the garment inputs['garment_torch']
    (nbatch,T,Vg,3) + inputs['smpl_root_joints_torch'] (nbatch,T,3), HIP tensors, as ONE mesh per frame -- the faces joined as
    render.render_output joins them (`body_model.faces`, then `garment_faces` (nfg,3) offset by Vb) --, body faces labelled 0, garment faces
    `garment_label`: the loader's label_dict[name] - 1 (utils/dataloader.py:15-23, 279), so Tshirt is 6.
    Returns {'pcd_torch': (nbatch,T,N,3), 'pcd_label_torch': (nbatch,T,N,1) int32, 'count': (nbatch,T) int32}, ready to be placed into
    `inputs`; the points are in scan order, not shuffled (see scan_meshes)."""
    body, cloth, root = (inputs[k] for k in ("smpl_vertices_torch", "garment_torch", "smpl_root_joints_torch"))
    if not all(torch.is_tensor(t) for t in (body, cloth, root)) or body.dim() != 4 or cloth.dim() != 4 or body.shape[-1] != 3 or cloth.shape[-1] != 3 \
            or cloth.shape[:2] != body.shape[:2] or root.numel() != body.shape[0] * body.shape[1] * 3:
        raise ValueError("scan_batch: smpl_vertices_torch (nbatch, T, Vb, 3), garment_torch (nbatch, T, Vg, 3) and smpl_root_joints_torch (nbatch, T, 3) expected")
    for name, t in (("smpl_vertices_torch", body), ("garment_torch", cloth), ("smpl_root_joints_torch", root)):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise TypeError(f"scan_batch: inputs['{name}'] must be a float32 HIP tensor (no CPU fallback)")
    nbatch, T, Vb = int(body.shape[0]), int(body.shape[1]), int(body.shape[2])
    verts = torch.cat([body, cloth + root.reshape(nbatch, T, 1, 3)], 2).reshape(nbatch * T, -1, 3)
    faces = render._joined_faces(body_model.faces, garment_faces, Vb)
    nfb = int(np.asarray(body_model.faces).shape[0])

    def labels():
        assert not torch.cuda.is_current_stream_capturing(), "scan: build the face labels before the capture (call once eagerly)"
        host = np.zeros(len(faces), np.int32)
        host[nfb:] = int(garment_label)
        return torch.from_numpy(host).to(body.device)
    face_labels = _cache.by_identity(_label_cache, 8, (faces,), (nfb, int(garment_label), str(body.device)), labels)
    s = scan_meshes(verts, faces, cameras if cameras is not None else ring_cameras(1), image_size, n_points, face_labels, seed)
    N = int(n_points)
    return {"pcd_torch": s.points.view(nbatch, T, N, 3), "pcd_label_torch": s.labels.view(nbatch, T, N, 1), "count": s.count.view(nbatch, T)}
