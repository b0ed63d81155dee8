"""float64 twin of the refinement head (modules/mesh_encoder.py:445-486) in plain torch on the CPU, differentiated by torch's autograd --
TEST INFRASTRUCTURE, shared by tests/test_refine_grad_cpu.py (which ties it to the reference's own float64 run through the figures stored in
tests/golden/refine_grad.npz) and tests/test_refine_grad_gpu.py (which holds the HIP training route to it).  Not a test module.

Same operations as the reference's loop, on point-major tensors: grouped rows [x_j - q ; f_j] -> Linear -> ReLU -> Linear -> max over the
samples; softmax(q k^T / sqrt(T)) v over the frames of a clip; A (X W) + b with ReLU between the four layers; residual update.  The ball
queries are the C oracle's on the fp32 rounding of the current vertices (indices are constants of the graph), as in the generator's
float64 run of the reference."""
import numpy as np
import torch

from garment4d_amd import mesh_utils, synthetic as syn
from oracle import gcn_oracle as GO
from oracle import pointnet2_oracle as K

BODY_R, BODY_S = (0.1, 0.2, 0.4), (8, 16, 32)
GARM_R, GARM_S = (0.1, 0.2, 0.4), (32, 16, 8)      # Tshirt
ENC = [f"{kind}_positional_encoding{i}" for kind in ("body", "garment") for i in range(3)]
PARAMS = [f"{e}.{l}.{w}" for e in ENC for l in (0, 2) for w in ("weight", "bias")] + ["temporal_qkv_1.weight", "temporal_qkv_2.weight"]
INPUTS = ["cur_garment_v"] + [f"garment_v_list{i}" for i in range(3)] + [f"garment_f_list{i}" for i in range(3)]
NAMES = PARAMS + INPUTS


def _encoder(sd, name, xyz, cur, feats, idx):
    F_ = xyz.shape[0]
    fi = torch.arange(F_)[:, None, None]
    ix = torch.from_numpy(idx.astype(np.int64))
    rows = torch.cat([xyz[fi, ix] - cur[:, :, None, :], feats[fi, ix]], -1)
    h = torch.relu(rows @ sd[f"{name}.0.weight"].T + sd[f"{name}.0.bias"])
    return (h @ sd[f"{name}.2.weight"].T + sd[f"{name}.2.bias"]).max(2)[0]


def forward(sd, cur, body_v, body_vn, gv, gf, A, nbatch, T, iteration=3):
    """sd: float64 tensors by the head's state-dict names; A dense (Vg,Vg).  Returns the list of refined vertices per round."""
    F_, Vg, _ = cur.shape
    outs, feats = [], []
    f32 = lambda t: np.ascontiguousarray(t.detach().numpy().astype(np.float32))
    for it in range(iteration):
        blocks = [cur]
        for i in range(3):
            idx = K.ball_query(BODY_R[i], BODY_S[i], f32(body_v), f32(cur))
            blocks.append(_encoder(sd, f"body_positional_encoding{i}", body_v, cur, body_vn, idx))
        for i in range(3):
            idx = K.ball_query(GARM_R[i], GARM_S[i], f32(gv[i]), f32(cur))
            blocks.append(_encoder(sd, f"garment_positional_encoding{i}", gv[i], cur, gf[i], idx))
        if it > 0:
            last = feats[-2].reshape(nbatch, T, Vg, -1)
            q, k, v = (last @ sd[f"temporal_qkv_{it}.weight"].T).chunk(3, dim=-1)
            q, k, v = (t.reshape(nbatch, T, -1) for t in (q, k, v))
            att = torch.softmax(q @ k.transpose(1, 2) / np.sqrt(T), dim=-1)
            blocks.append((att @ v).reshape(F_, Vg, -1))
        x = torch.cat(blocks, -1)
        for l in range(4):
            x = A @ (x @ sd[f"lbs_graph_regress{it + 1}.{l}.weight"]) + sd[f"lbs_graph_regress{it + 1}.{l}.bias"]
            if l < 3:
                x = torch.relu(x)
            feats.append(x)
        cur = cur + x
        outs.append(cur)
    return outs


def reference_gradients(case, golden_refine, gr):
    """{name: float64 numpy gradient} of sum_r <out_r, cot_r> for the fixture's inputs (tests/golden/refine_grad.npz holds the cotangents)."""
    nbatch, T = case["nbatch"], case["T"]
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    sd = {k: t64(v).requires_grad_(k in PARAMS) for k, v in syn.refine_state_dict(seed=case["seed"] + 100).items()}
    faces = case["body"]["faces"]
    body_v = t64(case["batch"]["smpl_vertices_torch"].reshape(nbatch * T, -1, 3))
    body_vn = t64(golden_refine["body_vn"])
    A = t64(GO.adjacency_from_faces(case["template_faces"], case["Vg"]).toarray().astype(np.float32))
    cur = t64(golden_refine["fwd_it3_lbs_pred"].reshape(nbatch * T, -1, 3)).requires_grad_(True)
    gv = [t64(v).requires_grad_(True) for v in case["garment_v_list"]]
    gf = [t64(f).requires_grad_(True) for f in case["garment_f_list"]]
    prev = K.set_contraction("nvcc")     # the mode the generator's runs (and the library by default) search in
    try:
        outs = forward(sd, cur, body_v, body_vn, gv, gf, A, nbatch, T)
    finally:
        K.set_contraction(prev)
    torch.autograd.backward(outs, [t64(gr[f"cot{r}"]) for r in range(3)])
    got = {k: sd[k].grad for k in PARAMS}
    got.update({"cur_garment_v": cur.grad}, **{f"garment_v_list{i}": gv[i].grad for i in range(3)}, **{f"garment_f_list{i}": gf[i].grad for i in range(3)})
    return {k: v.numpy() for k, v in got.items()}


def collect(head, cur, gv, gf):
    """The same names from a GarmentRefinementHead after backward()."""
    p = dict(head.named_parameters())
    got = {k: p[k].grad for k in PARAMS}
    got.update({"cur_garment_v": cur.grad}, **{f"garment_v_list{i}": gv[i].grad for i in range(3)}, **{f"garment_f_list{i}": gf[i].grad for i in range(3)})
    return got
