"""Drawing the predicted meshes on HIP: what utils/nr_utils.py:33-81 (`render_one_batch`) does with neural_renderer -- a look-at camera,
256 x 256 pixels, flat white faces under ambient + one directional light, 2 x anti-aliasing -- plus what that library does not hand out: a depth
image and the face index of every sample.  csrc/render/raster.hip (libg4d_render.so) is an exact-coverage tiled rasterizer: one projection
launch, one face-setup launch, one tile launch; include/g4d_render.h is its contract, tests/render_twin.py the numpy restatement.

neural_renderer is a CUDA extension that is not available to this project: pixel parity with it is NOT claimed.  Camera and light follow its
documented defaults; coverage, depth and shading are defined by the header.  No atomics, no host round trip and no allocation inside the calls:
after one eager call (which copies `faces` to the host once per faces object, for the index check) a call can be captured in a hipGraph.
There is no fallback: without the library, or on a CPU tensor, the calls raise."""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _cache
from . import _lib

Camera = collections.namedtuple("Camera", "eye at up half_angle near")
Rendered = collections.namedtuple("Rendered", "image depth face_id")
Projected = collections.namedtuple("Projected", "px py invz cam")

# neural_renderer's defaults (Renderer.__init__): viewing_angle 30, near 0.1, light_intensity_ambient / _directional 0.5, light_direction (0, 1, 0)
VIEWING_ANGLE, NEAR, AMBIENT, DIRECTIONAL, LIGHT_DIRECTION = 30.0, 0.1, 0.5, 0.5, (0.0, 1.0, 0.0)


def chunk():
    """Faces per chunk of the tile kernel's walk (g4d_render_chunk)."""
    return int(_lib.render_lib()[0].g4d_render_chunk())


def look_at_camera(distance, elevation, azimuth, half_angle=VIEWING_ANGLE, near=NEAR):
    """The camera of `renderer.eye = nr.get_points_from_angles(distance, elevation, azimuth)` (degrees) in camera_mode 'look_at': it looks at
    the origin with +y up.  eye = (d cos(el) sin(az), d sin(el), -d cos(el) cos(az))."""
    el, az = math.radians(elevation), math.radians(azimuth)
    return Camera((distance * math.cos(el) * math.sin(az), distance * math.sin(el), -distance * math.cos(el) * math.cos(az)), (0.0, 0.0, 0.0),
                  (0.0, 1.0, 0.0), float(half_angle), float(near))


def camera_rotation(camera):
    """The rows (x, y, z) of the look-at basis in float64, by the header's formula (z towards `at`, x = up X z, y = z X x)."""
    eye, at, up = (np.asarray(np.asarray(a, np.float32), np.float64) for a in (camera.eye, camera.at, camera.up))
    unit = lambda a: a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    z = unit(at - eye)
    x = unit(np.cross(up, z))
    return np.stack([x, unit(np.cross(z, x)), z])


def _size(image_size):
    w, h = (image_size, image_size) if np.isscalar(image_size) else image_size
    return int(w), int(h)


def _f32(name, t, shape_tail):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape[-len(shape_tail):]) == shape_tail):
        raise TypeError(f"{name}: a float32 HIP tensor of shape (..., {', '.join(map(str, shape_tail))}) expected (no CPU fallback)")
    return t.contiguous()


def project(verts, camera, image_size=256, ss=2, frames=None):
    """g4d_render_project_f32: verts (F,V,3), or (V,3) shared by `frames` frames -> Projected(px (F,V) int32, py, invz (F,V), cam (F,V,3))."""
    v = _f32("project: verts", verts, (3,))
    shared = v.dim() == 2
    if v.dim() not in (2, 3) or (shared and frames is None):
        raise ValueError("project: verts must be (F, V, 3), or (V, 3) together with frames=")
    F_, V = (int(frames), v.shape[0]) if shared else (v.shape[0], v.shape[1])
    w, h = _size(image_size)
    dev = v.device
    out = Projected(torch.empty((F_, V), dtype=torch.int32, device=dev), torch.empty((F_, V), dtype=torch.int32, device=dev),
                    torch.empty((F_, V), dtype=torch.float32, device=dev), torch.empty((F_, V, 3), dtype=torch.float32, device=dev))
    _lib.render_lib()
    _lib.call("g4d_render_project_f32", F_, V, int(shared), v.data_ptr(), *map(float, camera.eye), *map(float, camera.at), *map(float, camera.up),
              float(camera.half_angle), float(camera.near), w, h, int(ss), out.px.data_ptr(), out.py.data_ptr(), out.invz.data_ptr(),
              out.cam.data_ptr(), _lib.stream_ptr())
    return out


_faces_cache = {}


def _faces(faces, device):
    """(device int32 (nf,3), host int32 array) of a faces object, once per object: the host copy is what the entry point checks the indices on."""
    def build():
        assert not torch.cuda.is_current_stream_capturing(), "render: copy the faces before the capture (call once eagerly)"
        f = np.ascontiguousarray((faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int32))
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("render: faces must be (nf, 3) triangles")
        return torch.from_numpy(f).to(device), f

    return _cache.by_identity(_faces_cache, 16, (faces,), str(device), build)


def rasterize(px, py, invz, faces, image_size=256, ss=2, cam=None, face_colours=None, vertex_colours=None, light=(0.0, 0.0, 0.0), ambient=1.0,
              directional=0.0, background=(0.0, 0.0, 0.0), cull=True, want_image=True, kept=None):
    """g4d_render_raster on integer positions: px, py (F,V) int32 in 1/256 of a sample, invz (F,V), faces (nf,3) shared by the frames ->
    Rendered(image (F,H,W,3) or None, depth (F,ss H,ss W), face_id (F,ss H,ss W) int32).  `light` is the light's direction in CAMERA space and
    shades only when `cam` (F,V,3) is given.  cull=False tests every face against every tile (same bits).  kept: an int32 tensor of
    F * ceil(ss H / 16) * ceil(ss W / 16) entries that receives the number of faces each tile kept (measurement)."""
    for name, t, dt in (("px", px, torch.int32), ("py", py, torch.int32), ("invz", invz, torch.float32)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.dim() == 2 and t.shape == px.shape):
            raise TypeError(f"rasterize: {name} must be a {dt} HIP tensor of shape (F, V) (no CPU fallback)")
    px, py, invz = px.contiguous(), py.contiguous(), invz.contiguous()
    F_, V = px.shape
    dev = px.device
    w, h = _size(image_size)
    f_dev, f_host = _faces(faces, dev)
    nf = int(f_host.shape[0])
    if cam is not None:
        cam = _f32("rasterize: cam", cam, (V, 3))
    if face_colours is not None:
        face_colours = _f32("rasterize: face_colours", face_colours, (nf, 3))
    if vertex_colours is not None:
        vertex_colours = _f32("rasterize: vertex_colours", vertex_colours, (V, 3))
    L, _, _ = _lib.render_lib()
    nbytes = int(L.g4d_render_ws_bytes(F_, nf))
    ws = _lib.workspace(nbytes, dev)
    face_id = torch.empty((F_, ss * h, ss * w), dtype=torch.int32, device=dev)
    depth = torch.empty((F_, ss * h, ss * w), dtype=torch.float32, device=dev)
    image = torch.empty((F_, h, w, 3), dtype=torch.float32, device=dev) if want_image else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.call("g4d_render_raster", F_, V, nf, w, h, int(ss), int(bool(cull)), px.data_ptr(), py.data_ptr(), invz.data_ptr(), ptr(cam), f_dev.data_ptr(),
              f_host.ctypes.data_as(ctypes.c_void_p), ptr(face_colours), ptr(vertex_colours), *map(float, light), float(ambient), float(directional),
              *map(float, background), ws.data_ptr(), ws.numel(), face_id.data_ptr(), depth.data_ptr(), ptr(image), ptr(kept), _lib.stream_ptr())
    return Rendered(image, depth, face_id)


def render_meshes(verts, faces, camera=None, face_colours=None, vertex_colours=None, light_direction=LIGHT_DIRECTION, ambient=AMBIENT,
                  directional=DIRECTIONAL, background=(0.0, 0.0, 0.0), image_size=256, anti_aliasing=True):
    """verts (F,V,3) in world space, faces (nf,3) shared by the frames -> Rendered(image (F,H,W,3) in [0, 1] for colours in [0, 1], depth and
    face_id (F,ss H,ss W), ss = 2 with anti-aliasing, else 1).  Flat shading, both sides lit: intensity = ambient + directional * max(0, n . l)
    with the face normal turned towards the viewer and l = `light_direction` (world space).  Colours: white, or `face_colours` (nf,3), or
    `vertex_colours` (V,3) interpolated perspective-correct.  depth is the camera-space z of the visible surface, +inf on the background;
    face_id its face, -1 on the background.  Faces with a vertex nearer than the camera's `near`, and zero-area faces, are not drawn
    (nothing is clipped)."""
    camera = camera if camera is not None else look_at_camera(1.5, 0.0, 45.0)
    ss = 2 if anti_aliasing else 1
    p = project(_f32("render_meshes: verts", verts, (3,)), camera, image_size, ss)
    light = (camera_rotation(camera) @ np.asarray(light_direction, np.float64)).astype(np.float32)
    return rasterize(p.px, p.py, p.invz, faces, image_size, ss, cam=p.cam, face_colours=face_colours, vertex_colours=vertex_colours, light=light,
                     ambient=ambient, directional=directional, background=background)


def error_colours(pred, gt, lo, hi):
    """Per-vertex colours in [0, 1] of the distance |pred - gt| (..., V, 3) -> (..., V, 3) by the `rgb` ramp of utils/post_processing.py:260-269:
    ratio = 2 (value - lo) / (hi - lo); b = max(0, int(255 (1 - ratio))), r = max(0, int(255 (ratio - 1))), g = 255 - b - r (int truncates
    towards zero); blue at lo, green half way, red at hi.  Returned as (r, g, b) / 255."""
    value = (pred - gt).norm(dim=-1)
    ratio = 2.0 * (value - float(lo)) / (float(hi) - float(lo))
    b = (255.0 * (1.0 - ratio)).trunc().clamp_min(0.0)
    r = (255.0 * (ratio - 1.0)).trunc().clamp_min(0.0)
    return torch.stack([r, 255.0 - b - r, b], -1) / 255.0


_AXIS_SWAP = ((1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))   # nr_utils.py:64-68: vertices @ rot_mat


def render_output(output_dict, inputs, body_model, add_cloth=False):
    """render_one_batch (utils/nr_utils.py:33-81) on a forward's result: the body of inputs['pose_torch'] (nbatch,T,72) / inputs['beta_torch']
    (nbatch,T,10) from `body_model` (this package's body_models.SMPLLayer), with add_cloth the last refinement round
    output_dict['iter_regressed_lbs_garment_v'][-1] and output_dict['garment_f_3'] appended (faces offset by the body's vertex count), both
    through the axis swap of :64-68, camera distance 1.5, elevation 0, azimuth 45, white faces.
    Returns the reference's tuple: images (nbatch,T,256,256,3) float32 scaled by 256 and capped at 255 (the reference maps 256 to 255), body vertices (nbatch,T,V,3),
    body faces (nbatch,T,nf,3) int32, garment vertices (nbatch,T,Vg,3), garment faces (nbatch,T,nfg,3) -- numpy, like the reference's.  (The
    reference reads the garment for its return value also without add_cloth, where it has not defined it; here it is returned either way.)"""
    from .lbs import batch_rodrigues
    nbatch, T = inputs["pose_torch"].shape[0], inputs["pose_torch"].shape[1]
    dev = body_model.shapedirs.device
    pose = inputs["pose_torch"].reshape(-1, 72).to(device=dev, dtype=torch.float32)
    beta = inputs["beta_torch"].reshape(-1, 10).to(device=dev, dtype=torch.float32)
    rot = batch_rodrigues(pose.reshape(-1, 3).contiguous()).view(-1, 24, 3, 3)
    so = body_model(betas=beta.contiguous(), body_pose=rot[:, 1:], global_orient=rot[:, 0].reshape(-1, 1, 3, 3), pose2rot=False)
    body_v = so["vertices"]
    body_f = np.ascontiguousarray(np.asarray(body_model.faces).astype(np.int32))
    cloth_v = output_dict["iter_regressed_lbs_garment_v"][-1].reshape(nbatch * T, -1, 3).to(device=dev, dtype=torch.float32)
    cloth_f = np.ascontiguousarray(np.asarray(output_dict["garment_f_3"]).astype(np.int32))
    verts, faces = body_v, body_model.faces      # (the model's own object: its device copy is cached by identity)
    if add_cloth:
        verts = torch.cat([body_v, cloth_v], 1)
        faces = _joined_faces(body_model.faces, output_dict["garment_f_3"], body_v.shape[1])
    verts = torch.matmul(verts, torch.tensor(_AXIS_SWAP, dtype=torch.float32, device=dev))
    # :74-75 scale by 256 and map 256 to 255; values in (255, 256) are taken down to 255 with it, so that the range is 0..255 as a float
    # array too (the reference's save_images truncates to uint8, which gives the same picture)
    images = np.minimum(render_meshes(verts, faces, look_at_camera(1.5, 0.0, 45.0)).image.cpu().numpy() * 256, np.float32(255))
    F_ = nbatch * T
    tile = lambda f: np.broadcast_to(f[None], (F_,) + f.shape).reshape(nbatch, T, -1, 3)
    return (images.reshape(nbatch, T, 256, 256, 3), body_v.cpu().numpy().reshape(nbatch, T, -1, 3), tile(body_f),
            cloth_v.cpu().numpy().reshape(nbatch, T, -1, 3), tile(cloth_f))


_joined_cache = {}


def _joined_faces(body_faces, cloth_faces, nbody):
    """Body faces followed by the garment's, offset by the body's vertex count (:59): one array per pair of faces objects."""
    return _cache.by_identity(_joined_cache, 8, (body_faces, cloth_faces), int(nbody),
                              lambda: np.ascontiguousarray(np.concatenate([np.asarray(body_faces).astype(np.int32),
                                                                           np.asarray(cloth_faces).astype(np.int32) + int(nbody)], 0)))
