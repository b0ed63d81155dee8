"""Time garment post-processing (garment4d_amd/postprocess.py) at the BASELINE cfg4 shape: 240 frames (8 clips x 30), a 64 x 64 = 4096-vertex
garment around the SMPL-sized body of scripts/time_model.py (65 x 106 = 6890 vertices, 13568 faces = 212 blocks of 64).
usage: python scripts/time_postprocess.py [frames] [iters] [cpu_frames]

Prints per-stage device times (HIP events around each stage, median of `iters` after one warm-up), the nearest-point search with and without
the box cull and the share of face blocks the culled search goes through, the whole post_process call eager and as one hipGraph replay, and
-- as the reference-style baseline -- the float64 numpy / scipy twin (tests/postprocess_twin.py) on the CPU for `cpu_frames` frames.
The last line is one JSON object with every figure."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from garment4d_amd import _lib, gcn, postprocess as pp, synthetic as syn, tuning

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 240
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cpu_frames = int(sys.argv[3]) if len(sys.argv) > 3 else 1
BODY_RC, GARMENT_RC = (65, 106), (64, 64)


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


assert torch.cuda.is_available(), "time_postprocess.py measures on the GPU; there is no CPU fallback"
rng = np.random.default_rng(1)
bv0, bq = syn.quad_cylinder(*BODY_RC)
body_faces = tris(bq)
body_np = np.stack([pose(bv0, f) for f in range(frames)])
_, gq = syn.quad_cylinder(*GARMENT_RC)
garment_faces = tris(gq)
adj_old = gcn.adjacency_old_from_faces(gq, GARMENT_RC[0] * GARMENT_RC[1])
r = (np.arange(GARMENT_RC[0]) * BODY_RC[0]) // GARMENT_RC[0]
c = (np.arange(GARMENT_RC[1]) * BODY_RC[1]) // GARMENT_RC[1]
sel = (r[:, None] * BODY_RC[1] + c[None, :]).reshape(-1)
garment_np = syn.garment_around_body(rng, body_np, syn.vertex_normals(body_np, body_faces), sel)
body_v, garment_v = torch.from_numpy(body_np).cuda(), torch.from_numpy(garment_np).cuda()
F_, Vg, V, nf = frames, garment_v.shape[1], body_v.shape[1], len(body_faces)
nblocks, waves = (nf + 63) // 64, frames * ((Vg + 63) // 64)
res = dict(frames=F_, Vg=Vg, V=V, faces=nf, face_blocks=nblocks, point_triangle_tests_per_round=F_ * Vg * nf)

res["taubin_ms"], smooth = timed(lambda: pp.taubin_smooth(garment_v, adj_old))
res["body_prepass_ms"], body = timed(lambda: pp._SearchMesh(body_v, body_faces))                 # vertex normals + block boxes, once per call
gtopo = pp.mesh_topology(garment_faces, Vg, garment_v.device, smooth[0])
res["garment_normals_ms"], m = timed(lambda: pp.vertex_normals_area(smooth, gtopo))
visited = torch.zeros(waves, dtype=torch.int32, device="cuda")
res["nearest_culled_ms"], near = timed(lambda: body.nearest(smooth, visited=visited))
res["blocks_visited_share"] = float(visited.float().mean()) / nblocks
with tuning.use(tuning.current().replace(nearest_cull=False)):
    res["nearest_unculled_ms"], near_all = timed(lambda: body.nearest(smooth))
assert all(torch.equal(a, b) for a, b in zip(near, near_all)), "cull on / off differ"
res["nearest_unculled_tests_per_s"] = res["point_triangle_tests_per_round"] / (res["nearest_unculled_ms"] * 1e-3)
w2 = torch.empty((F_, Vg), device="cuda")
target = torch.empty((F_, Vg, 3), device="cuda")
counts = torch.empty(F_, dtype=torch.int32, device="cuda")
st = _lib.stream_ptr()
res["targets_ms"], _ = timed(lambda: _lib.call("g4d_depen_targets_f32", F_, Vg, 0.008, 2.0, smooth.data_ptr(), near.point.data_ptr(), near.normal.data_ptr(),
                                               m.data_ptr(), None, w2.data_ptr(), target.data_ptr(), counts.data_ptr(), st))
op = pp.depenetration_operator(adj_old, garment_v.device)
solved, resid = torch.empty_like(smooth), torch.empty((F_, 3), device="cuda")
res["solve_32_iters_ms"], _ = timed(lambda: _lib.call("g4d_depen_solve_f32", F_, Vg, 32, op[7], op[8], smooth.data_ptr(), w2.data_ptr(), target.data_ptr(),
                                                      counts.data_ptr(), *[t.data_ptr() for t in op[:6]], solved.data_ptr(), resid.data_ptr(), st))
res["solve_residual_max"] = float(resid.max())
res["flagged_share_round0"] = float(counts.float().mean()) / Vg
res["post_process_eager_ms"], out = timed(lambda: pp.post_process(garment_v, garment_faces, body_v, body_faces, adj_old))
res["counts_per_round_mean"] = [float(x) for x in out[1].float().mean(1)]
res["residual_max"] = float(out[2].max())
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    pp.post_process(garment_v, garment_faces, body_v, body_faces, adj_old)
torch.cuda.current_stream().wait_stream(side)
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    captured = pp.post_process(garment_v, garment_faces, body_v, body_faces, adj_old)
res["post_process_graph_ms"], _ = timed(graph.replay)
assert torch.equal(captured[0], out[0]), "graph replay differs from eager"

if cpu_frames > 0:
    import postprocess_twin as tw
    t0 = time.perf_counter()
    tv, tc = tw.post_process(garment_np[:cpu_frames], garment_faces, body_np[:cpu_frames], body_faces, adj_old)
    res["cpu_twin_float64_s_per_frame"] = (time.perf_counter() - t0) / cpu_frames
    res["cpu_twin_rounds_run"] = [int((tc[:, f] > 0).sum()) + 1 for f in range(cpu_frames)]
    res["max_abs_diff_to_cpu_twin"] = float(np.abs(out[0][:cpu_frames].cpu().numpy() - tv).max())
for k, v in res.items():
    print(f"{k}: {v}")
print(json.dumps(res))
