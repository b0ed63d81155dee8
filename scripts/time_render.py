"""Time the rasterizer (garment4d_amd/render.py, csrc/render/raster.hip) at BASELINE cfg4's mesh sizes: 240 frames of a 6890-vertex body plus a
4096-vertex garment (13568 + 8064 faces), 256 x 256 pixels at 2 x 2 samples, the reference's camera after its axis swap.
usage: python scripts/time_render.py [frames] [iters] [twin]
Prints the time of one render_meshes call (HIP events around `iters` calls), the share of each entry point, the number of faces a tile keeps
(cull on / off) and -- with `twin` -- the CPU time of the numpy twin (tests/render_twin.py) for one frame, for scale."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from garment4d_amd import _lib, render
from garment4d_amd import synthetic as syn

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 240
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
with_twin = len(sys.argv) > 3 and sys.argv[3] == "twin"
T = 30
nbatch = (frames + T - 1) // T

scene = syn.garment_scene(nbatch, T, 4, body_rc=(65, 106), garment_rc=(64, 64), seed=1)
body_v = scene["batch"]["smpl_vertices_torch"].reshape(-1, 6890, 3)[:frames]
gv, gq = scene["template"]
rng = np.random.default_rng(2)
cloth_v = (gv[None] + np.cumsum(rng.standard_normal((frames, 1, 3)) * 0.004, 0) + rng.standard_normal((frames,) + gv.shape) * 0.001).astype(np.float32)
faces = np.concatenate([scene["body"]["faces"], np.concatenate([gq[:, [0, 1, 2]], gq[:, [0, 2, 3]]], 0) + 6890]).astype(np.int32)
verts = np.concatenate([body_v, cloth_v], 1) @ np.array(render._AXIS_SWAP, np.float32)
camera = render.look_at_camera(1.5, 0.0, 45.0)
v = torch.from_numpy(np.ascontiguousarray(verts)).cuda()

for _ in range(2):
    out = render.render_meshes(v, faces, camera)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(iters):
    out = render.render_meshes(v, faces, camera)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / iters
with _lib.timed_calls() as t:
    render.render_meshes(v, faces, camera)
parts = ", ".join(f"{name} {us / 1e3:.2f} ms" for name, _, us in t.results())
seen = out.face_id >= 0
print(f"frames={frames} V={verts.shape[1]} faces={len(faces)} 256x256 ss=2: {ms:.2f} ms / call ({frames / ms * 1e3:.0f} frames/s); {parts}; "
      f"covered samples {float(seen.float().mean()):.3f}, body faces seen {int((out.face_id[seen] < 13568).sum())}, garment {int((out.face_id[seen] >= 13568).sum())}")

p = render.project(v, camera, 256, 2)
tiles = frames * 32 * 32
for cull in (True, False):
    kept = torch.zeros(tiles, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e0.record()
    r = render.rasterize(p.px, p.py, p.invz, faces, 256, 2, cam=p.cam, light=(0.0, 1.0, 0.0), ambient=0.5, directional=0.5, cull=cull, kept=kept)
    e1.record()
    torch.cuda.synchronize()
    k = kept.float()
    print(f"cull={int(cull)}: raster {e0.elapsed_time(e1):.2f} ms; faces kept per tile: mean {float(k.mean()):.1f}, max {int(k.max())}, "
          f"over tiles with any {float(k[k > 0].mean()):.1f} ({float((k > 0).float().mean()):.2f} of the tiles); same ids as the default: {bool(torch.equal(r.face_id, out.face_id))}")

if with_twin:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import render_twin as RT
    cam = RT.camera(camera.eye, camera.at, camera.up, camera.half_angle, 256, 256, 2)
    t0 = time.perf_counter()
    px, py, invz, c = RT.project_f32(verts[0], cam, camera.near)
    tw = RT.raster(px, py, invz, faces, 512, 512, 2, cam=c, light=RT.light_in_camera(cam, render.LIGHT_DIRECTION), ambient=0.5, directional=0.5)
    dt = time.perf_counter() - t0
    print(f"numpy twin, one frame on the CPU: {dt:.2f} s; face ids equal the kernel's: {bool(np.array_equal(tw['face_id'], out.face_id[0].cpu().numpy()))}; "
          f"depth bits equal: {bool(np.array_equal(tw['depth'].view(np.int32), out.depth[0].cpu().numpy().view(np.int32)))}")
