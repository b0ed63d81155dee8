"""Time forward + backward of the GCN layer at the cfg4 shape (8 clips x 30 frames x 4096 garment vertices = 983 040 rows) on one GPU:
  hip     the autograd route of garment4d_amd/gcn.py (tuning.Tuning.gcn_autograd): forward launches + csrc/gcn_grad.hip
  torch   the same layers written from the layer's formula  Y = act(Ahat (X W) + b)  as torch.matmul + torch.sparse.mm (batch folded into
          the columns) + torch's autograd on the same GPU -- what a user had to fall back to before the backward kernels existed
for 323 -> 128, 128 -> 128 (both with the ReLU of the regressor loop), 128 -> 3 and the whole stack 323 -> 128 -> 128 -> 128 -> 3; gradients
of the input and of every parameter are asked for in both routes.  Device events around `iters` calls after a warm-up, the median is printed.
Per launch (from _lib.timed_calls): g4d_gemm_tn_f32 against its two floors, 2 rows Fin Cout flop at the 157 TFLOP/s fp32 MFMA peak and
rows (Fin + Cout) 4 bytes at the 8 TB/s HBM peak.
usage: python scripts/time_gcn_grad.py [frames] [side] [iters]      (Vg = side x side quad cylinder)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from garment4d_amd import _lib, tuning
from garment4d_amd import gcn as G
from garment4d_amd import synthetic as syn

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 240
side = int(sys.argv[2]) if len(sys.argv) > 2 else 64
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
assert torch.cuda.is_available(), "time_gcn_grad.py measures on the GPU"
PEAK_FLOPS, PEAK_BYTES = 157e12, 8e12


def timed(fn, n=iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


_, faces = syn.quad_cylinder(side, side)
Vg = side * side
adj_sp = G.adjacency_from_faces(faces, Vg)
adj = G.sparse_mx_to_torch_sparse_tensor(adj_sp)
adj_dev = adj.cuda().coalesce()
rows = frames * Vg
torch.manual_seed(0)


def torch_layer(x, W, b, relu):
    B, N, _ = x.shape
    s = torch.matmul(x, W)
    y = torch.sparse.mm(adj_dev, s.transpose(0, 1).reshape(N, -1)).reshape(N, B, -1).transpose(0, 1) + b
    return torch.relu(y) if relu else y


def case(widths):
    layers = [G.GraphConvolution(a, b).cuda() for a, b in zip(widths[:-1], widths[1:])]
    n = len(layers)
    x = torch.randn(frames, Vg, widths[0], device="cuda").requires_grad_(True)
    dy = torch.randn(frames, Vg, widths[-1], device="cuda")
    relu_last = n == 1 and widths[-1] == 128   # a single hidden layer is timed with the ReLU that follows it in the regressor loop
    params = [p for m in layers for p in (m.weight, m.bias)]

    def hip():
        with tuning.use(tuning.current().replace(gcn_autograd=True)):
            y = G.gcn_stack_forward(layers, x, adj, relu_last=relu_last)[-1]
        return torch.autograd.grad(y, [x] + params, dy)

    def ref():
        h = x
        for i, m in enumerate(layers):
            h = torch_layer(h, m.weight, m.bias, i + 1 < n or relu_last)
        return torch.autograd.grad(h, [x] + params, dy)

    ga, gb = hip(), ref()
    # the two routes' fp32 forwards put a handful of the 126 M near-zero pre-activations on different sides of the ReLU, and one flip moves
    # the gradients behind it by a discrete amount (percent of the maximum in dX): the routes are compared with each other AND, for a single
    # layer, each with a float64 backward under its OWN forward's mask
    res = dict(widths=list(widths), hip_vs_torch_max_rel=max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(ga, gb)))
    if n == 1:
        m = layers[0]
        with torch.no_grad():
            with tuning.use(tuning.current().replace(gcn_autograd=False)):
                yh = m(x.detach(), adj, relu=relu_last)
            yt = torch_layer(x.detach(), m.weight, m.bias, relu_last)
            res["relu_flips_between_routes"] = int(((yh > 0) != (yt > 0)).sum()) if relu_last else 0
            for name, y, got in (("hip", yh, ga), ("torch", yt, gb)):
                g = dy.double() * (y > 0) if relu_last else dy.double()
                ds = torch.sparse.mm(adj_dev.double().t(), g.transpose(0, 1).reshape(Vg, -1)).reshape(Vg, frames, -1).transpose(0, 1)
                want = (ds @ m.weight.double().t(), x.detach().double().reshape(rows, -1).t() @ ds.reshape(rows, -1), g.reshape(rows, -1).sum(0))
                res[name + "_vs_float64_max_rel"] = max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(got, want))
                del g, ds, want
            del yh, yt
    del ga, gb
    torch.cuda.empty_cache()
    res.update(hip_ms=timed(hip)[0], torch_ms=timed(ref)[0])
    res["speedup"] = res["torch_ms"] / res["hip_ms"]
    with _lib.timed_calls() as t:
        for _ in range(3):
            hip()
    per = {}
    for name, ints, us in t.results():
        per.setdefault((name, ints[:4]), []).append(us)
    launches = []
    for (name, ints), us in per.items():
        row = dict(call=name, args=list(ints), us=float(np.median(us)))
        if name == "g4d_gemm_tn_f32":
            r, fin, _, cout = ints
            row["mfma_floor_us"] = 2.0 * r * fin * cout / PEAK_FLOPS * 1e6
            row["hbm_floor_us"] = 4.0 * r * (fin + cout) / PEAK_BYTES * 1e6
            row["fraction_of_mfma_floor"] = row["mfma_floor_us"] / row["us"]
            row["fraction_of_hbm_floor"] = row["hbm_floor_us"] / row["us"]
        launches.append(row)
    res["launches"] = launches
    return res


out = dict(shape=dict(frames=frames, Vg=Vg, rows=rows), cases=[])
for widths in ((323, 128), (128, 128), (128, 3), (323, 128, 128, 128, 3)):
    out["cases"].append(case(widths))
    torch.cuda.empty_cache()
print(json.dumps(out))
