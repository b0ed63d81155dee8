"""The refinement head's training route (tuning.Tuning.refine_autograd): csrc/pos_encode_grad.hip and csrc/attention_grad.hip, each alone
against the float64 twin of tests/refine_grad_twin.py with bounds derived there (nothing in them is a measured number), the head's wiring,
and the reference's own autograd through tests/golden/refine_grad.npz.

Discrete decisions.  A max-pool argmax or a ReLU whose float64 margin is at rounding level may fall either way in two correct fp32
evaluations.  The twin alone flags every (query, channel) whose top-two margin between distinct source points, or whose winning row's smallest
|pre-activation|, is below MARGIN = 4 x the forward error bound of the case; the cotangent is set to zero there on both sides.  The flagged
share must stay below 1 % in every case (asserted; the inputs change if it does not, never the cap)."""
import numpy as np
import pytest
import torch

import refine_grad_twin as TW
from garment4d_amd import _lib, fused, tuning
from garment4d_amd import gcn as G
from garment4d_amd import mesh_utils, synthetic as syn
from garment4d_amd import refine as R
from garment4d_amd.refine import GarmentRefinementHead
from oracle import gcn_oracle as GO

pytestmark = pytest.mark.gpu
PE_OUTPUTS = ("dW1", "db1", "dW2", "db2", "d_new_xyz", "d_xyz", "d_extra", "d_table")
ATOMIC_FREE = ("dW1", "db1", "dW2", "db2", "d_new_xyz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def refine_on():
    return tuning.use(tuning.current().replace(refine_autograd=True))


# ---- positional encoder -------------------------------------------------------------------------------------------------------------------
pe_case = TW.pe_case   # shared with tests/test_pos_encode_gpu.py


def hip_pe_grad(c, dOut, ldg=32, col0=0, want=PE_OUTPUTS):
    """One raw launch; outputs not in `want` (or not defined for the case) get a null pointer.  Returns {name: numpy}."""
    F_, N, P, S, E = c["F"], c["N"], c["P"], c["S"], c["E"]
    t = {k: (None if c[k] is None else dev(c[k])) for k in ("xyz", "new_xyz", "extra", "table", "idx", "W1", "b1", "W2")}
    buf = torch.zeros((F_, P, ldg), device="cuda")
    buf[..., col0:col0 + 32] = dev(dOut)
    shapes = dict(dW1=(32, 3 + E), db1=(32,), dW2=(32, 32), db2=(32,), d_new_xyz=(F_, P, 3), d_xyz=(F_, N, 3), d_extra=(F_, N, E), d_table=(F_, N, 32))
    out = {}
    for k in want:
        if (k == "d_extra" and not E) or (k == "d_table" and c["table"] is None):
            continue
        out[k] = torch.zeros(shapes[k], device="cuda") if k in ("d_xyz", "d_extra", "d_table") else torch.full(shapes[k], float("nan"), device="cuda")
    ws = torch.empty(max(int(_lib.lib().g4d_pos_encode_grad_ws_bytes(F_, P, S)) // 4, 1), device="cuda")
    P_ = lambda x: 0 if x is None else x.data_ptr()
    _lib.call("g4d_pos_encode_grad_f32", F_, N, P, S, E, P_(t["xyz"]), P_(t["new_xyz"]), P_(t["extra"]), P_(t["table"]), P_(t["idx"]), P_(t["W1"]),
              P_(t["b1"]), P_(t["W2"]), buf.data_ptr(), ldg, col0, ws.data_ptr(), *[P_(out.get(k)) for k in PE_OUTPUTS], _lib.stream_ptr())
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


def reduction_depth(F_, P, S):
    """Depth of the documented reduction tree of dW1 / db1 / dW2 / db2 (csrc/pos_encode_grad.hip): a lane's chain over its wave's iterations
    (64 pairs each for dW1), the two halves, the waves of a workgroup, the workgroup partials in four chains."""
    nblocks = int(_lib.lib().g4d_pos_encode_grad_ws_bytes(F_, P, S)) // 4 // (32 * 32 + 32 + 32 * 8 + 32)
    waves = 2 if S > 32 else 4
    pairs = (F_ * P + 1) // 2
    iters = -(-pairs // (nblocks * waves))
    return iters * 64 + 1 + waves + (nblocks + 3) // 4 + 3


def twin_pe(c):
    """(grads, bounds, flagged share, dOut with the flagged entries zeroed), frame by frame so that the full-size case fits."""
    F_, N, E = c["F"], c["N"], c["E"]
    kx = 3 + E
    def forward(f):
        s = slice(f, f + 1)
        return TW.pe_forward(c["xyz"][s], c["new_xyz"][s], None if c["extra"] is None else c["extra"][s], None if c["table"] is None else c["table"][s],
                             c["idx"][s], c["W1"], c["b1"], c["W2"], c["b2"])
    margin = max(4.0 * TW.forward_error_bound(forward(f), c["W2"]) for f in range(F_))   # of the whole case; the forwards are recomputed below
    dOut = c["dOut"].astype(np.float64).copy()
    G, B = {}, {}
    depth = reduction_depth(F_, c["P"], c["S"])
    flagged = 0
    parts = []
    for f in range(F_):
        fw = forward(f)
        fl = TW.pe_flags(fw, margin)
        flagged += int(fl.sum())
        dOut[f][fl[0]] = 0.0
        parts.append(TW.pe_backward(fw, c["W1"], c["W2"], dOut[f:f + 1], N, E, c["table"] is not None))
    cnt_w = {"dW2": F_ * c["P"], "db2": F_ * c["P"], "dW1": sum(p[2]["dW1"] for p in parts), "db1": sum(p[2]["db1"] for p in parts)}
    for k in parts[0][0]:
        if k in cnt_w:
            G[k] = sum(p[0][k] for p in parts)
            B[k] = TW.bound(cnt_w[k], sum(p[1][k] for p in parts), kx, depth=depth)
        else:
            G[k] = np.concatenate([p[0][k] for p in parts], 0)
            B[k] = np.concatenate([TW.bound(p[2][k], p[1][k], kx) for p in parts], 0)
    return G, B, flagged / (F_ * c["P"] * 32.0), dOut.astype(np.float32), margin


def check_pe(c, what, **kw):
    G, B, share, dOut, margin = twin_pe(c)
    print(f"{what}: MARGIN {margin:.3e}, flagged share {share:.5f}")
    assert share <= 0.01, f"{what}: {share:.4f} of the (query, channel) pairs are flagged (cap 1 %): change the inputs"
    got = hip_pe_grad(c, dOut, **kw)
    assert set(got) == set(G), (sorted(got), sorted(G))
    for k in sorted(G):
        err = np.abs(got[k].astype(np.float64) - G[k])
        worst = float((err / np.maximum(B[k], 1e-300)).max())
        print(f"{what} {k}: max err / bound = {worst:.3f}, max |ref| = {np.abs(G[k]).max():.3e}")
        assert not (err > B[k]).any(), f"{what} {k}: {int((err > B[k]).sum())} of {err.size} elements beyond the derived bound (worst ratio {worst:.3f})"
        assert np.abs(G[k]).max() > 0
    return got, dOut


@pytest.mark.parametrize("S", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("variant", ["plain0", "plain3", "plain5", "table"])
def test_pos_encode_grad_against_float64(S, variant):
    E = {"plain0": 0, "plain3": 3, "plain5": 5, "table": 0}[variant]
    c = pe_case(100 + S + 7 * E + (1000 if variant == "table" else 0), 2, 301, 259, S, E, variant == "table")
    check_pe(c, f"S={S} {variant}", ldg=40, col0=5)


@pytest.mark.parametrize("variant", ["plain3", "table"])
def test_pos_encode_grad_padding_heavy(variant):
    """Most rows are copies of the first hit (at most 3 distinct hits out of 32): ties among copies go to the same source point."""
    c = pe_case(77, 2, 301, 259, 32, 3 if variant == "plain3" else 0, variant == "table", hits=3)
    assert (c["idx"][..., 3:] == c["idx"][..., :1]).all()
    check_pe(c, f"padding-heavy {variant}")


def test_pos_encode_grad_full_cfg4_launch():
    """The launch size of one body encoder at cfg4: 240 frames x 4096 queries x 8 samples over 6890 body vertices with normals."""
    c = pe_case(5, 240, 6890, 4096, 8, 3, False)
    check_pe(c, "cfg4 body encoder S=8", ldg=196, col0=3)


def test_pos_encode_grad_reproducible_and_skippable():
    """Two runs agree bit for bit on every output specified as atomic-free; asking for fewer outputs leaves the others' bits alone."""
    for variant in ("plain3", "table"):
        c = pe_case(11, 3, 500, 700, 16, 3 if variant == "plain3" else 0, variant == "table")
        a = hip_pe_grad(c, c["dOut"])
        b = hip_pe_grad(c, c["dOut"])
        for k in ATOMIC_FREE:
            assert np.array_equal(a[k], b[k]), (variant, k)
        for want in (("dW2",), ("db1", "d_new_xyz"), ("dW1", "db2", "d_xyz"), ("d_new_xyz",), ("d_table", "dW2")):
            s = hip_pe_grad(c, c["dOut"], want=want)
            for k in s:
                if k in ATOMIC_FREE:   # (the atomic scatter-adds are the same sums in another order: held to the twin above, not compared here)
                    assert np.array_equal(s[k], a[k]), (variant, want, k)


# ---- temporal attention -------------------------------------------------------------------------------------------------------------------
def hip_attention(qkv, n_clips, T, Vg, C):
    res = torch.empty((n_clips * T, Vg, C), device="cuda")
    scratch = torch.empty(_lib.lib().g4d_temporal_attention_scratch_floats(n_clips, Vg, C), device="cuda")
    att = torch.empty((n_clips, T, T), device="cuda")
    _lib.call("g4d_temporal_attention_f32", n_clips, T, Vg, C, qkv.data_ptr(), scratch.data_ptr(), att.data_ptr(), res.data_ptr(), C, 0, _lib.stream_ptr())
    return res, att


def hip_attention_grad(qkv, att, dbuf, ldg, col0, n_clips, T, Vg, C):
    dqkv = torch.full_like(qkv, float("nan"))
    scratch = torch.empty(_lib.lib().g4d_temporal_attention_grad_scratch_floats(n_clips, Vg, C), device="cuda")
    _lib.call("g4d_temporal_attention_grad_f32", n_clips, T, Vg, C, qkv.data_ptr(), att.data_ptr(), dbuf.data_ptr(), ldg, col0, scratch.data_ptr(),
              dqkv.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return dqkv


def check_attention(seed, n_clips, T, Vg, C, ldg, col0, scale):
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.randn((n_clips * T, Vg, 3 * C), device="cuda", generator=g) * scale
    dbuf = torch.randn((n_clips * T, Vg, ldg), device="cuda", generator=g)
    _, att = hip_attention(qkv, n_clips, T, Vg, C)
    dqkv = hip_attention_grad(qkv, att, dbuf, ldg, col0, n_clips, T, Vg, C)
    again = hip_attention_grad(qkv, att, dbuf, ldg, col0, n_clips, T, Vg, C)
    assert torch.equal(dqkv, again), "the attention backward is specified as bit-reproducible"
    worst = 0.0
    for c in range(n_clips):   # clip by clip: the full-size case does not fit as one float64 array
        s = slice(c * T, (c + 1) * T)
        fw = TW.att_forward(host(qkv[s]), T)
        att_c = host(att[c:c + 1]).astype(np.float64)
        assert np.abs(att_c - fw["att"]).max() <= 1e-3, "the saved attention matrix is not the forward's"
        ref, bnd = TW.att_backward(fw, host(dbuf[s][..., col0:col0 + C]), att=att_c)
        err = np.abs(host(dqkv[s]).astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(bnd, 1e-300)).max()))
        assert not (err > bnd).any(), f"clip {c}: {int((err > bnd).sum())} of {err.size} elements beyond the derived bound (worst ratio {worst:.3f})"
        assert np.abs(ref).max() > 0
    print(f"attention grad T={T} Vg={Vg} C={C} clips={n_clips}: max err / bound = {worst:.3f}")


@pytest.mark.parametrize("T", [1, 3, 30, 32])
def test_attention_grad_against_float64(T):
    """D = Vg * C = 37 * 48 is not a multiple of a wave's slice (512 columns) nor of a workgroup's (2048); the cotangent sits at column 5 of
    rows padded to 61 floats."""
    check_attention(20 + T, 2, T, 37, 48, 61, 5, 0.15)


def test_attention_grad_full_size():
    check_attention(9, 8, 30, 4096, 128, 128, 0, 0.004)


# ---- the head -----------------------------------------------------------------------------------------------------------------------------
def small_head(iteration=3, seed=0):
    case = syn.refine_golden_case()
    nbatch, T = case["nbatch"], case["T"]
    head = GarmentRefinementHead(garment_name="Tshirt", iteration=iteration)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in syn.refine_state_dict(seed=case["seed"] + 100).items()}, strict=True)
    head = head.cuda().eval()
    faces = case["body"]["faces"]
    fid, vid = mesh_utils.calc_mesh_info(faces, case["body"]["v_template"].shape[0])
    body_v = dev(case["batch"]["smpl_vertices_torch"].reshape(nbatch * T, -1, 3))
    adj = G.sparse_mx_to_torch_sparse_tensor(GO.adjacency_from_faces(case["template_faces"], case["Vg"])).cuda()
    with torch.no_grad():
        body_vn = mesh_utils.compute_vnorms(body_v, torch.from_numpy(faces), vid, fid)
    return case, head, body_v, body_vn, adj


def head_inputs(case, golden_refine=None):
    nbatch, T = case["nbatch"], case["T"]
    if golden_refine is not None:
        cur = dev(golden_refine["fwd_it3_lbs_pred"].reshape(nbatch * T, -1, 3))
    else:
        cur = dev(np.tile(case["tpose_garment"][:, None], (1, T, 1, 1)).reshape(nbatch * T, -1, 3))
    return cur, [dev(v) for v in case["garment_v_list"]], [dev(f) for f in case["garment_f_list"]]


def test_head_trains_under_the_switch(golden_refine):
    g, _ = golden_refine
    case, head, body_v, body_vn, adj = small_head()
    nbatch, T = case["nbatch"], case["T"]
    cur, gv, gf = head_inputs(case, g)
    with torch.no_grad():
        want = head(cur, body_v, body_vn, gv, gf, adj, nbatch, T)
    with pytest.raises(AssertionError):    # off: as it always was
        head(cur, body_v, body_vn, gv, gf, adj, nbatch, T)
    cur.requires_grad_(True)
    for t in gv + gf:
        t.requires_grad_(True)
    with refine_on():
        outs = head(cur, body_v, body_vn, gv, gf, adj, nbatch, T)
        with pytest.raises(NotImplementedError):
            head(cur, body_v, body_vn, gv, gf, adj, nbatch, T, group="world")
    assert len(outs) == len(want) == 3
    for a, b in zip(outs, want):
        assert torch.equal(a.detach(), b), "the training route's forward is the inference route's bits"
    torch.manual_seed(1)
    loss = sum((o * torch.randn_like(o)).sum() for o in outs)
    loss.backward()
    for name, p in head.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), name
        assert p.grad.abs().max() > 0, name
    for name, t in [("cur_garment_v", cur)] + [(f"garment_v_list[{i}]", t) for i, t in enumerate(gv)] + [(f"garment_f_list[{i}]", t) for i, t in enumerate(gf)]:
        assert t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0, name
    with pytest.raises(AssertionError):    # and off again outside the block
        head(cur, body_v, body_vn, gv, gf, adj, nbatch, T)


def test_training_route_forward_bits_on_a_ragged_mesh():
    """195 garment vertices (13 x 15): the positional encoders' 64-row chunks straddle frames; the training route's forward is still the
    inference route's, bit for bit."""
    rng = np.random.default_rng(31)
    nbatch, T, V = 2, 3, 700
    F_ = nbatch * T
    verts, faces = syn.quad_cylinder(13, 15)
    Vg = verts.shape[0]
    assert Vg == 195 and all((Vg * s) % 64 for s in (4, 8, 16, 32))
    body_v = dev((syn.unit_cloud(F_, V, seed=32) - 0.5).astype(np.float32) * 0.8)
    body_vn = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((F_, V, 3)).astype(np.float32)), dim=-1).cuda()
    cur = (body_v[:, torch.from_numpy(rng.permutation(V)[:Vg]).cuda()] + dev(rng.standard_normal((F_, Vg, 3)).astype(np.float32)) * 0.03).contiguous()
    gv, gf = [], []
    for n, c in ((512, 64), (128, 96), (32, 384)):
        sel = torch.from_numpy(rng.integers(0, Vg, n)).cuda()
        gv.append((cur[:, sel] + dev(rng.standard_normal((F_, n, 3)).astype(np.float32)) * 0.05).contiguous())
        gf.append(dev(rng.standard_normal((F_, n, c)).astype(np.float32)))
    adj = G.sparse_mx_to_torch_sparse_tensor(GO.adjacency_from_faces(faces, Vg)).cuda()
    torch.manual_seed(31)
    head = GarmentRefinementHead(garment_name="Tshirt").cuda().eval()
    with torch.no_grad():
        for p in head.parameters():
            p.mul_(0.5)
        want = head(cur, body_v, body_vn, gv, gf, adj, nbatch, T)
    cur.requires_grad_(True)
    with refine_on():
        outs = head(cur, body_v, body_vn, gv, gf, adj, nbatch, T)
    assert len(outs) == len(want) == 3 and outs[-1].requires_grad
    for a, b in zip(outs, want):
        assert torch.equal(a.detach(), b), "the training route's forward is the inference route's bits"


def test_generic_encoder_shapes_have_no_backward():
    mlp = torch.nn.Sequential(torch.nn.Linear(3 + 3, 32), torch.nn.ReLU(), torch.nn.Linear(32, 32)).cuda()
    xyz, q, f = torch.randn(2, 50, 3, device="cuda"), torch.randn(2, 40, 3, device="cuda", requires_grad=True), torch.randn(2, 50, 3, device="cuda")
    idx = torch.zeros((2, 40, 12), dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError, match="nsample 12"):
        R._positional_encoding_autograd(mlp, 12, xyz, q, f, idx, None)


def test_head_gradients_against_the_reference_autograd(golden_refine):
    """tests/golden/refine_grad.npz: the reference's own refinement loop under torch's autograd on the CPU.  Per tensor
    max |hip - ref64| <= 3 e_ref, e_ref = max |ref32 - ref64| the reference's own fp32 error (the rule and margin of gcn_grad.npz); ref64 is
    recomputed by the float64 twin, which tests/test_refine_grad_cpu.py ties to the stored figures."""
    import refine_head_twin as HT
    gr = TW.load()
    g, _ = golden_refine
    case, head, body_v, body_vn, adj = small_head()
    nbatch, T = case["nbatch"], case["T"]
    cur, gv, gf = head_inputs(case, g)
    cur.requires_grad_(True)
    for t in gv + gf:
        t.requires_grad_(True)
    with refine_on():
        outs = head(cur, body_v, body_vn, gv, gf, adj, nbatch, T)
    torch.autograd.backward(outs, [dev(gr[f"cot{r}"]) for r in range(3)])
    ref64 = HT.reference_gradients(case, g, gr)
    got = HT.collect(head, cur, gv, gf)
    ratios = {}
    for name, ref in ref64.items():
        e = float(np.abs(host(got[name]).astype(np.float64) - ref).max())
        ratios[name] = e / float(gr[f"eref_{name}"])
        print(f"{name}: max |hip - ref64| = {e:.3e}, e_ref = {float(gr[f'eref_{name}']):.3e}, ratio {ratios[name]:.2f}")
    bad = {k: round(v, 2) for k, v in ratios.items() if v > 3.0}
    assert not bad, f"beyond 3 e_ref: {bad}"
