#!/usr/bin/env python
"""Generate tests/golden/refine_grad.npz: gradients of the REFERENCE's own refinement loop (`PCALBSGarmentUseSegEncoderSeg.forward`,
modules/mesh_encoder.py:445-486, three rounds) from torch's autograd on the CPU, in fp32 and through a float64 copy of the same model.

Run from the repo root:  G4D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_refine_grad.py
(its own process; G4D_GOLDEN_OUT=<dir> writes elsewhere, to compare).  Needs no GPU.  Only DATA is written.

Same stand-ins as make_golden_refine.py (whose loader this script imports), inputs from garment4d_amd/synthetic.py:refine_golden_case.  Two
more, both outside what is differentiated here:
  * `lbs_garment_interpolation` returns the LBS-posed garment stored in refine.npz (`fwd_it3_lbs_pred`, the reference's own output) as a
    LEAF, so that both precisions start the loop from the same vertices and d loss / d cur_garment_v is that leaf's gradient;
  * in the float64 run `pointnet2_utils.grouping_operation` is oracle/autograd_twin.py's float64 grouping (the extension's is fp32-only) and
    `ball_query` runs on the fp32 rounding of its arguments (indices are constants of the graph, QueryAndGroup).
Loss: sum over the three rounds of <iter_regressed_lbs_garment_v[r], cot_r> with fixed random cotangents (stored).

Stored: cot0..2; per tensor of refine_head_twin.NAMES (all encoder Linears, both qkv weights, cur_garment_v, garment_v_list, garment_f_list
-- the latter point-major) the fp32 gradient, eref_<name> = max |fp32 - float64| and max64_<name> = max |float64|.  The GCN weights are
pinned by gcn_grad.npz and left out (file size).  eref contains the reference's own coin tosses -- an argmax, a ReLU or a ball query that
falls differently in the two precisions -- which no seed removes at this size; `decisions` = [ball-query index entries, encoder ReLU signs,
max-pool argmaxes, GCN ReLU signs] that differ between the two runs, `decisions_total` the number of each."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.environ.get("G4D_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")

spec = importlib.util.spec_from_file_location("make_golden_refine", os.path.join(ROOT, "tests", "golden", "make_golden_refine.py"))
MG = importlib.util.module_from_spec(spec)
spec.loader.exec_module(MG)

from garment4d_amd import synthetic as syn  # noqa: E402
from oracle import autograd_twin as AT  # noqa: E402
from oracle import pointnet2_oracle as K  # noqa: E402
import refine_head_twin as HT  # noqa: E402

T_, N_ = MG.T, MG.N


def run(me, case, ref, cots, dt):
    """One forward + backward of the reference model in dtype dt.  Returns ({name: gradient}, decision records)."""
    pu = importlib.import_module("modules.pointnet2.pointnet2.pointnet2_utils") if "modules.pointnet2.pointnet2.pointnet2_utils" in sys.modules \
        else next(m for n, m in sys.modules.items() if n.endswith("pointnet2_utils") and hasattr(m, "QueryAndGroup"))
    nbatch, Tn = case["nbatch"], case["T"]
    model = MG.build_model(me, case, iteration=3)
    faces = case["body"]["faces"]
    vf_vid = np.concatenate([faces[:, c] for c in range(3)])
    vf_fid = np.concatenate([np.arange(faces.shape[0])] * 3)
    model.vf_fid, model.vf_vid = T_(vf_fid.astype(np.int64)), T_(vf_vid.astype(np.int64))
    rec = dict(bq=[], relu=[], argmax=[], gcn=[])
    saved = dict(bq=pu.ball_query, group=pu.grouping_operation, relu=me.F.relu)
    if dt == torch.float64:
        model = model.double()
        model.adj = model.adj.double()
        pu.grouping_operation = lambda feats, idx: AT.grouping_operation(feats.double(), idx)   # (fp32 constants -- body vertices, normals -- promoted exactly)
        orig_bq = saved["bq"]
        pu.ball_query = lambda r, s, xyz, new_xyz: orig_bq(r, s, xyz.detach().float().contiguous(), new_xyz.detach().float().contiguous())
    inner_bq = pu.ball_query

    def bq(r, s, xyz, new_xyz):
        idx = inner_bq(r, s, xyz, new_xyz)
        rec["bq"].append(N_(idx).copy())
        return idx
    pu.ball_query = bq

    def relu(x, *a, **k):
        rec["gcn"].append(N_(x > 0).copy())
        return saved["relu"](x, *a, **k)
    me.F.relu = relu
    hooks = []
    for seq in list(model.body_positional_encoding_list) + list(model.garment_positional_encoding_list):
        hooks.append(seq[1].register_forward_hook(lambda m, i, o: rec["relu"].append(N_(o > 0).copy())))
        hooks.append(seq.register_forward_hook(lambda m, i, o: rec["argmax"].append(N_(o.argmax(-2)).copy())))
    cur = T_(ref["fwd_it3_lbs_pred"]).to(dt).requires_grad_(True)
    model.lbs_garment_interpolation = lambda *a, **k: (cur, None, None)
    gv = [T_(v).to(dt).requires_grad_(True) for v in case["garment_v_list"]]
    gf = [T_(np.ascontiguousarray(np.transpose(f, (0, 2, 1)))).to(dt).requires_grad_(True) for f in case["garment_f_list"]]
    model.PCA_garment_encoder.out = dict(garment_v_list=gv, garment_f_list=gf, tpose_garment=T_(case["tpose_garment"]).reshape(nbatch, -1))
    batch = {k: T_(v) for k, v in case["batch"].items()}
    body_model = types.SimpleNamespace(parents=T_(case["body"]["parents"]), faces=faces, J_regressor=T_(case["body"]["J_regressor"]))
    try:
        od = model(torch.zeros(nbatch, Tn, 4, 3), body_model, batch)
        outs = od["iter_regressed_lbs_garment_v"]
        torch.autograd.backward(outs, [T_(c).to(dt) for c in cots])
    finally:
        pu.ball_query, pu.grouping_operation, me.F.relu = saved["bq"], saved["group"], saved["relu"]
        for h in hooks:
            h.remove()
    p = dict(model.named_parameters())
    # the reference keeps its sub-modules in lists; the head's names are the state-dict keys of garment4d_amd.refine.GarmentRefinementHead
    grads = {k: p[k].grad for k in HT.PARAMS}
    grads["cur_garment_v"] = cur.grad.reshape(nbatch * Tn, -1, 3)
    for i in range(3):
        grads[f"garment_v_list{i}"] = gv[i].grad
        grads[f"garment_f_list{i}"] = gf[i].grad.transpose(1, 2)
    return {k: N_(v).copy() for k, v in grads.items()}, rec, [N_(o).copy() for o in outs]


def main():
    torch.set_num_threads(1)
    K.set_contraction("nvcc")
    me = MG.load_reference()
    case = syn.refine_golden_case()
    ref = np.load(os.path.join(ROOT, "tests", "golden", "refine.npz"))
    assert np.array_equal(ref["checksum"], syn.refine_golden_checksum(case)), "refine.npz belongs to other inputs"
    rng = np.random.default_rng(case["seed"] + 300)
    F_ = case["nbatch"] * case["T"]
    cots = [rng.standard_normal((F_, case["Vg"], 3)).astype(np.float32) for _ in range(3)]
    g32, rec32, outs32 = run(me, case, ref, cots, torch.float32)
    g64, rec64, _ = run(me, case, ref, cots, torch.float64)
    for r in range(3):   # the fp32 run is the run refine.npz stores
        assert np.array_equal(outs32[r], ref[f"fwd_it3_round{r}"]), r
    out = {f"cot{r}": c for r, c in enumerate(cots)}
    for k in HT.NAMES:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64 and g32[k].shape == g64[k].shape, k
        out[k] = g32[k]
        out[f"eref_{k}"] = np.float64(np.abs(g32[k].astype(np.float64) - g64[k]).max())
        out[f"max64_{k}"] = np.float64(np.abs(g64[k]).max())
    kinds = ("bq", "relu", "argmax", "gcn")
    for kind in kinds:
        assert len(rec32[kind]) == len(rec64[kind]) and len(rec32[kind]) > 0, kind
    out["decisions"] = np.array([sum(int((a != b).sum()) for a, b in zip(rec32[k], rec64[k])) for k in kinds], dtype=np.int64)
    out["decisions_total"] = np.array([sum(a.size for a in rec32[k]) for k in kinds], dtype=np.int64)
    out["checksum"] = syn.refine_golden_checksum(case)
    path = os.path.join(OUT, "refine_grad.npz")
    np.savez_compressed(path, **out)
    print("refine_grad.npz", len(out), "arrays", os.path.getsize(path), "bytes; decisions differing", out["decisions"], "of", out["decisions_total"])
    for k in HT.NAMES:
        print(f"  {k}: eref {float(out['eref_' + k]):.3e}  max64 {float(out['max64_' + k]):.3e}")


if __name__ == "__main__":
    main()
