"""Time forward + backward of the refinement head at the cfg4 shape (8 clips x 30 frames, 4096 garment / 6890 body vertices, three rounds)
and of each new backward kernel alone, on one GPU:
  hip     GarmentRefinementHead under tuning.Tuning.refine_autograd: the inference launches + csrc/pos_encode_grad.hip,
          csrc/attention_grad.hip and csrc/gcn_grad.hip
  torch   the same computation as plain torch ops + torch's autograd on the same GPU, in the reference's grouped-row formulation
          (modules/mesh_encoder.py:445-486): gather the (query, sample) rows [x_j - q ; f_j], Linear -> ReLU -> Linear, max over the samples;
          softmax(q k^T / sqrt(T)) v with torch.matmul; the GCN layers as torch.matmul + torch.sparse.mm.  Both routes use the SAME ball-query
          indices (the package's), gradients of cur_garment_v and of every parameter are asked for in both.
Device events around each call after a warm-up; median and minimum are printed.  Per launch (from _lib.timed_calls):
  g4d_temporal_attention_grad_f32 against the bytes it must move, eight (T, D) blocks (dO and V once, Q, K and dO once, three written),
    at the 8 TB/s HBM peak;
  g4d_pos_encode_grad_f32 as grouped rows per second and as the share of the fp32 vector peak (157 TFLOP/s) of the FMAs of the recomputed
    forward and the sparse backward (rows (3 + E + 32) + queries 32 (64 + 2 (3 + E)) FMAs for all 32 channels).
usage: python scripts/time_refine_grad.py [clips] [T] [side] [iters] [torch: 0|1]      (Vg = side x side)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from garment4d_amd import _lib, fused, tuning
from garment4d_amd import gcn as G
from garment4d_amd import synthetic as syn
from garment4d_amd.refine import GarmentRefinementHead

clips = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 30
side = int(sys.argv[3]) if len(sys.argv) > 3 else 64
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 5
with_torch = (int(sys.argv[5]) if len(sys.argv) > 5 else 1) != 0
assert torch.cuda.is_available(), "time_refine_grad.py measures on the GPU"
PEAK_FLOPS, PEAK_BYTES = 157e12, 8e12
F_, Vg, V = clips * T, side * side, 6890


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


torch.manual_seed(0)
_, faces = syn.quad_cylinder(side, side)
adj = G.sparse_mx_to_torch_sparse_tensor(G.adjacency_from_faces(faces, Vg))
adj_dev = adj.cuda().coalesce()
head = GarmentRefinementHead().cuda().eval()
with torch.no_grad():   # untrained regressors move the vertices out of every ball after one round (all ball queries then fall back to point 0 and every
    for reg in (head.lbs_graph_regress1, head.lbs_graph_regress2, head.lbs_graph_regress3):   # scatter-add lands on one row): keep the update small
        reg[3].weight.mul_(0.02)
        reg[3].bias.mul_(0.02)
body_v = torch.rand(F_, V, 3, device="cuda")
body_vn = torch.nn.functional.normalize(torch.randn(F_, V, 3, device="cuda"), dim=-1)
cur0 = (body_v[:, torch.randint(0, V, (Vg,), device="cuda")] + torch.randn(F_, Vg, 3, device="cuda") * 0.02).contiguous()
gv = [(cur0[:, torch.randint(0, Vg, (n,), device="cuda")] + torch.randn(F_, n, 3, device="cuda") * 0.01).contiguous() for n in (2048, 512, 64)]
gf = [torch.randn(F_, n, c, device="cuda") for n, c in ((2048, 64), (512, 96), (64, 384))]
params = list(head.parameters())
cots = [torch.randn(F_, Vg, 3, device="cuda") for _ in range(3)]
on = tuning.current().replace(refine_autograd=True)


def hip_head():
    cur = cur0.clone().requires_grad_(True)
    with tuning.use(on):
        outs = head(cur, body_v, body_vn, gv, gf, adj, clips, T)
    return torch.autograd.grad(outs, [cur] + params, cots)


def torch_encoder(seq, xyz, cur, feats, idx):
    fi = torch.arange(F_, device="cuda")[:, None, None]
    ix = idx.long()
    rows = torch.cat([xyz[fi, ix] - cur[:, :, None, :], feats[fi, ix]], -1)
    return seq(rows).max(2)[0]


def torch_attention(lin, x):
    q, k, v = lin(x.reshape(clips, T, Vg, -1)).chunk(3, dim=-1)
    q, k, v = (t.reshape(clips, T, -1) for t in (q, k, v))
    att = torch.softmax(torch.matmul(q, k.transpose(1, 2)) / (T ** 0.5), dim=-1)
    return torch.matmul(att, v).reshape(F_, Vg, -1)


def torch_gcn(m, x, relu):
    s = torch.matmul(x, m.weight)
    y = torch.sparse.mm(adj_dev, s.transpose(0, 1).reshape(Vg, -1)).reshape(Vg, F_, -1).transpose(0, 1) + m.bias
    return torch.relu(y) if relu else y


def torch_head():
    body_pe = [head.body_positional_encoding0, head.body_positional_encoding1, head.body_positional_encoding2]
    garm_pe = [head.garment_positional_encoding0, head.garment_positional_encoding1, head.garment_positional_encoding2]
    regress = [head.lbs_graph_regress1, head.lbs_graph_regress2, head.lbs_graph_regress3]
    qkvs = [head.temporal_qkv_1, head.temporal_qkv_2]
    cur = cur0.clone().requires_grad_(True)
    leaf, outs, feats = cur, [], []
    for it in range(3):
        with torch.no_grad():
            bidx = fused.ball_query_msg(head.body_radius_list, head.body_sample_num_list, body_v, cur.detach().contiguous(), coherent=True)
            gidx = [fused.ball_query_msg([head.garment_radius_list[i]], [head.garment_sample_num_list[i]], gv[i], cur.detach().contiguous())[0] for i in range(3)]
        blocks = [cur] + [torch_encoder(body_pe[i], body_v, cur, body_vn, bidx[i]) for i in range(3)]
        blocks += [torch_encoder(garm_pe[i], gv[i], cur, gf[i], gidx[i]) for i in range(3)]
        if it > 0:
            blocks.append(torch_attention(qkvs[it - 1], feats[-2]))
        x = torch.cat(blocks, -1)
        for l, m in enumerate(regress[it]):
            x = torch_gcn(m, x, l < 3)
            feats.append(x)
        cur = cur + x
        outs.append(cur)
    return torch.autograd.grad(outs, [leaf] + params, cots)


out = dict(shape=dict(clips=clips, T=T, frames=F_, Vg=Vg, body=V, garment_levels=[2048, 512, 64]))
ga = hip_head()
out["head_hip_ms"], out["head_hip_min_ms"] = timed(hip_head)
if with_torch:
    gb = torch_head()
    # two correct fp32 forwards put a few argmaxes / ReLUs on different sides; the routes are compared loosely here, the tests hold each to float64
    out["head_hip_vs_torch_max_rel"] = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(ga, gb))
    del gb
    torch.cuda.empty_cache()
    out["head_torch_ms"], out["head_torch_min_ms"] = timed(torch_head, n=max(2, iters // 2), warm=1)
    out["head_speedup"] = out["head_torch_ms"] / out["head_hip_ms"]
del ga
torch.cuda.empty_cache()

with _lib.timed_calls() as t:
    for _ in range(3):
        hip_head()
per = {}
for name, ints, us in t.results():
    if name in ("g4d_pos_encode_grad_f32", "g4d_temporal_attention_grad_f32", "g4d_pos_encode_f32", "g4d_temporal_attention_f32"):
        per.setdefault((name, tuple(ints[:5])), []).append(us)
launches = []
for (name, ints), us in per.items():
    row = dict(call=name, args=list(ints), us=float(np.median(us)), launches_per_step=len(us) // 3)
    if name == "g4d_temporal_attention_grad_f32":
        nclips, t_, vg, c = ints[:4]
        row["bytes"] = 8.0 * nclips * t_ * vg * c * 4
        row["bytes_per_s"] = row["bytes"] / (row["us"] * 1e-6)
        row["fraction_of_hbm_peak"] = row["bytes_per_s"] / PEAK_BYTES
    if name == "g4d_pos_encode_grad_f32":
        frames, n, p, s, e = ints[:5]
        rows, q = frames * p * s, frames * p
        row["rows_per_s"] = rows / (row["us"] * 1e-6)
        row["fma"] = 32.0 * (rows * (3 + e + 32) + q * (64 + 2 * (3 + e)))   # (a table encoder: e = 0)
        row["fraction_of_valu_peak"] = 2.0 * row["fma"] / (row["us"] * 1e-6) / PEAK_FLOPS
    launches.append(row)
out["launches"] = sorted(launches, key=lambda r: (r["call"], r["args"]))


# each new kernel alone against its torch formulation: one body encoder (S = 32, normals), one table encoder (S = 32, 64 features), the attention
def encoder_alone(name, seq, xyz, feats, S, radius):
    with torch.no_grad():
        idx = fused.ball_query_msg([radius], [S], xyz, cur0)[0]
    ps = list(seq.parameters())
    dy = torch.randn(F_, Vg, 32, device="cuda")
    from garment4d_amd import refine as R

    def hip():
        cur = cur0.clone().requires_grad_(True)
        tab = R._FeatureTableFn.apply(feats, seq[0].weight[:, 3:], seq[0].bias, seq) if feats.shape[2] > 32 else None
        y = R._positional_encoding_autograd(seq, S, xyz, cur, feats, idx, tab)
        return torch.autograd.grad(y, [cur] + ps, dy)

    def ref():
        cur = cur0.clone().requires_grad_(True)
        return torch.autograd.grad(torch_encoder(seq, xyz, cur, feats, idx), [cur] + ps, dy)
    r = dict(case=name, hip_ms=timed(hip)[0])
    if with_torch:
        r["torch_ms"] = timed(ref, n=max(2, iters // 2), warm=1)[0]
        r["speedup"] = r["torch_ms"] / r["hip_ms"]
    torch.cuda.empty_cache()
    return r


def attention_alone():
    from garment4d_amd import dist as gdist
    lin = head.temporal_qkv_1
    x0 = torch.randn(F_, Vg, 128, device="cuda") * 0.05
    dy = torch.randn(F_, Vg, 128, device="cuda")

    def hip():
        x = x0.clone().requires_grad_(True)
        with tuning.use(on):
            y = gdist.temporal_attention(x, None, F_, T, head._qkv(lin), None, qkv_linear=lin)
        return torch.autograd.grad(y, [x, lin.weight], dy)

    def ref():
        x = x0.clone().requires_grad_(True)
        return torch.autograd.grad(torch_attention(lin, x), [x, lin.weight], dy)
    r = dict(case="temporal attention + qkv Linear", hip_ms=timed(hip)[0])
    if with_torch:
        r["torch_ms"] = timed(ref, n=max(2, iters // 2), warm=1)[0]
        r["speedup"] = r["torch_ms"] / r["hip_ms"]
    return r


out["alone"] = [encoder_alone("body encoder S=32, normals", head.body_positional_encoding2, body_v, body_vn, 32, 0.4),
                encoder_alone("garment encoder S=32, table of 64 features", head.garment_positional_encoding0, gv[0], gf[0], 32, 0.1),
                attention_alone()]
print(json.dumps(out))
