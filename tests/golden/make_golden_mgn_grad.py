#!/usr/bin/env python
"""Generate tests/golden/mgn_grad.npz: one training step's worth of the REFERENCE's MGN baseline on the CPU -- its own
`PCALBSGarmentUseSegEncoderSegMGN.forward` (modules/mesh_encoder.py:587-614), its `temporal_loss_PCA_LBS` (smplx/loss/temporal_loss.py:147-201)
and torch's autograd of `total_loss` -- once in fp32 and once in float64 on the same inputs.

Run from the repo root:  G4D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_mgn_grad.py
(its own process; G4D_GOLDEN_OUT=<dir> writes elsewhere, to compare).  Needs no GPU.  Only DATA is written.

Loader and stand-ins as make_golden_mgn.py (stub garment encoder returning the case's tpose_garment / garment_summary, `knn_points` ->
oracle/refine_oracle.knn_points, `.cuda` -> identity); loss set-up as make_golden_stage2_loss.py (`smplx.loss` registered as a package,
`utils.config.cfg.LOSS` = cfgs/tshirt.yaml's 20 / 10 / 100 / 5, the vertex-face incidence preset from the face list).  The float64 pass runs
under torch.set_default_dtype(torch.float64): the reference creates `inv_template_pose` with torch.zeros (:543).
Inputs: garment4d_amd/synthetic.py:mgn_golden_case, mgn_displacement_state_dict(seed + 100), mgn_grad_targets (targets placed around `fwd_posed`
of tests/golden/mgn.npz, the reference's own forward output for the case; the loss's body widened so that about half of the garment penetrates).

Stored (fp32 run) with eref_<key> = max |fp32 - float64| of the reference itself and max64_<key>: every scalar of loss_dict;
d_lbs_pred = d total_loss / d lbs_pred_garment_v (F,Vg,3); the three bias gradients in full; per weight gradient its row sums (cout), column sums
(cin) -- float64 sums of the entries -- and 4096 sampled entries (flat indices stored: sample_idx_<layer>) -- the full matrices are 2-4 MB each.  Also: `decisions` = [nearest body
vertex of the skinning, ReLU decisions of the two hidden layers, penetration signs, nearest body vertex of the loss] that differ between the two
precisions (asserted 0), `min_abs_preact` of the two hidden layers (fp32 run), `penetrating_share` (asserted within 20-80 %), checksum."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_refine as MR  # noqa: E402  (exits unless G4D_REFERENCE_DIR is set; puts the repository root on sys.path)

sys.path.insert(0, os.path.join(MR.ROOT, "tests"))
from garment4d_amd import synthetic as syn  # noqa: E402
from oracle import pointnet2_oracle as K  # noqa: E402
import stage2_loss_twin as TW  # noqa: E402

T, N = MR.T, MR.N
SCALARS = ("lbs_garment_msre", "only_lbs_garment_msre", "lbs_garment_l2_loss", "lbs_garment_lap_loss", "lbs_interpenetration_loss",
           "temporal_constraint_loss", "acceleration_error", "only_lbs_acceleration_error", "total_loss")
LAYERS = (0, 2, 4)
SAMPLES, SAMPLE_SEED = 4096, 191


def run(me, tl, case, targets, sd, dt):
    torch.set_default_dtype(dt)
    try:
        nbatch, Tn, Vg = case["nbatch"], case["T"], case["Vg"]

        class StubGarmentEncoder(torch.nn.Module):
            """Stands in for PCAGarmentEncoderSeg: template topology + a fixed output_dict."""
            def __init__(self, cfg=None, args=None):
                super().__init__()
                self.remesh_cylinder_f = case["template_faces"]
                self.garment_v_num = Vg
                self.out = None

            def forward(self, x, body_model):
                return dict(self.out)
        me.PCAGarmentEncoderSeg = StubGarmentEncoder
        model = me.PCALBSGarmentUseSegEncoderSegMGN(types.SimpleNamespace(GARMENT=types.SimpleNamespace(NAME="Tshirt")), types.SimpleNamespace())
        model.load_state_dict({k: T(v).to(dt) for k, v in sd.items()}, strict=True)
        model.eval()
        assert all(p.dtype == dt for p in model.parameters())
        body = case["body"]
        faces = body["faces"]
        body_model = types.SimpleNamespace(parents=T(body["parents"]), faces=faces, J_regressor=T(body["J_regressor"]).to(dt))
        batch = {k: T(v).to(dt) for k, v in case["batch"].items()}
        model.PCA_garment_encoder.out = dict(tpose_garment=T(case["tpose_garment"]).to(dt).reshape(nbatch, -1),
                                             garment_summary=T(case["garment_summary"]).to(dt))
        rec = dict(pre=[], sign=[], idx=[])
        hooks = [model.displacement_encoder[i].register_forward_hook(lambda m, inp, out: rec["pre"].append(N(inp[0]).copy())) for i in (1, 3)]
        od = model(torch.zeros(nbatch, Tn, 4, 3, dtype=dt), body_model, batch)
        for h in hooks:
            h.remove()
        assert od["lbs_pred_garment_v"].dtype == dt and len(od["iter_regressed_lbs_garment_v"]) == 1
        od["lbs_pred_garment_v"].retain_grad()
        tl.vf_vid = T(np.concatenate([faces[:, c] for c in range(3)]).astype(np.int64))
        tl.vf_fid = T(np.concatenate([np.arange(faces.shape[0])] * 3).astype(np.int64))
        saved = (tl.F.relu, tl.knn_points)

        def relu(x, *a, **k):
            rec["sign"].append(N(x > 0).copy())
            return saved[0](x, *a, **k)

        def knn(p1, p2, *a, **k):
            out = saved[1](p1, p2, *a, **k)
            rec["idx"].append(N(out.idx).copy())
            return out
        tl.F.relu, tl.knn_points = relu, knn
        try:
            inputs = dict(pose_torch=batch["pose_torch"], smpl_vertices_torch=T(targets["smpl_vertices_torch"]).to(dt),
                          smpl_root_joints_torch=T(targets["smpl_root_joints_torch"]).to(dt), garment_torch=T(targets["garment_torch"]).to(dt),
                          garment_template_vertices=torch.zeros(nbatch, Vg, 3, dtype=dt))   # read at :172, its result never used
            od["lap_adj"] = od["lap_adj"].to(dt)
            ld = tl.temporal_loss_PCA_LBS(od, inputs, body_model, types.SimpleNamespace())
            ld["total_loss"].backward()
        finally:
            tl.F.relu, tl.knn_points = saved
        assert all(p.grad is not None and p.grad.dtype == dt for p in model.displacement_encoder.parameters())
        grads = {"d_lbs_pred": N(od["lbs_pred_garment_v"].grad).reshape(nbatch * Tn, Vg, 3).copy()}
        for i in LAYERS:
            grads[f"db{i}"] = N(model.displacement_encoder[i].bias.grad).copy()
            grads[f"dW{i}"] = N(model.displacement_encoder[i].weight.grad).copy()
        return {k: N(v).copy() for k, v in ld.items()}, grads, rec, N(od["lbs_nn"].idx).copy(), N(od["lbs_pred_garment_v"]).copy()
    finally:
        torch.set_default_dtype(torch.float32)


def weight_views(dw, sample):
    """Row / column sums accumulated in float64 (of the fp32 entries, for the fp32 run: no rounding of the summary's own) and the sampled entries."""
    return {"rowsum": dw.astype(np.float64).sum(1), "colsum": dw.astype(np.float64).sum(0), "sample": dw.reshape(-1)[sample]}


def main():
    torch.set_num_threads(1)
    K.set_contraction("nvcc")
    me = MR.load_reference()
    MR._pkg("smplx.loss", os.path.join(MR.REF, "smplx", "loss"))
    cfg = sys.modules["utils.config"].cfg
    cfg.LOSS = types.SimpleNamespace(**dict(zip(("LBS_GARMENT_L2_LOSS_LAMBDA", "LBS_GARMENT_LAP_LOSS_LAMBDA", "LBS_INTERPENETRATION_LOSS_LAMBDA",
                                                 "TEMPORAL_CONSTRAINT_LOSS_LAMBDA"), TW.LAMBDAS)))
    tl = importlib.import_module("smplx.loss.temporal_loss")
    case = syn.mgn_golden_case()
    Vg = case["Vg"]
    posed = np.load(os.path.join(MR.ROOT, "tests", "golden", "mgn.npz"))["fwd_posed"]
    targets = syn.mgn_grad_targets(case, posed)
    sd = syn.mgn_displacement_state_dict(Vg, seed=case["seed"] + 100)
    d32, g32, rec32, nn32, p32 = run(me, tl, case, targets, sd, torch.float32)
    d64, g64, rec64, nn64, p64 = run(me, tl, case, targets, sd, torch.float64)
    np.testing.assert_allclose(p32, posed, rtol=1e-5, atol=1e-6)       # the targets sit around this run's own prediction
    out = {}

    def put(key, a32, a64):
        assert a64.dtype == np.float64 and a32.shape == a64.shape, key
        out[key] = a32
        out[f"eref_{key}"] = np.float64(np.abs(a32.astype(np.float64) - a64).max())
        out[f"max64_{key}"] = np.float64(np.abs(a64).max())
    for k in SCALARS:
        assert d32[k].shape == (), k
        put(k, d32[k], d64[k])
    put("d_lbs_pred", g32["d_lbs_pred"], g64["d_lbs_pred"])
    rng = np.random.default_rng(SAMPLE_SEED)
    for i in LAYERS:
        put(f"db{i}", g32[f"db{i}"], g64[f"db{i}"])
        sample = np.sort(rng.choice(g32[f"dW{i}"].size, SAMPLES, replace=False)).astype(np.int64)
        out[f"sample_idx_{i}"] = sample
        v32, v64 = weight_views(g32[f"dW{i}"], sample), weight_views(g64[f"dW{i}"], sample)
        for name in v32:
            put(f"dW{i}_{name}", v32[name], v64[name])
    assert len(rec32["pre"]) == len(rec64["pre"]) == 2 and len(rec32["sign"]) == len(rec64["sign"]) == 1 and len(rec32["idx"]) == len(rec64["idx"]) == 1
    out["decisions"] = np.array([int((nn32 != nn64).sum()), sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(rec32["pre"], rec64["pre"])),
                                 int((rec32["sign"][0] != rec64["sign"][0]).sum()), int((rec32["idx"][0] != rec64["idx"][0]).sum())], dtype=np.int64)
    out["min_abs_preact"] = np.array([float(np.abs(a).min()) for a in rec32["pre"]])
    out["active_share"] = np.array([float((a > 0).mean()) for a in rec32["pre"]])
    out["penetrating_share"] = np.float64(rec32["sign"][0].mean())
    print("decisions", out["decisions"], "penetrating", out["penetrating_share"])
    assert (out["decisions"] == 0).all(), out["decisions"]
    assert 0.2 <= out["penetrating_share"] <= 0.8, out["penetrating_share"]
    out["target_seed"] = np.int64(190)
    out["checksum"] = syn.mgn_grad_checksum(case, targets)
    path = os.path.join(MR.OUT, "mgn_grad.npz")
    np.savez_compressed(path, **out)
    print("mgn_grad.npz", len(out), "arrays", os.path.getsize(path), "bytes; penetrating", out["penetrating_share"], "min |pre-activation|",
          out["min_abs_preact"], "active", out["active_share"])
    for k in out:
        if k.startswith("eref_"):
            print(f"  {k[5:]}: eref {float(out[k]):.3e}  max64 {float(out['max64_' + k[5:]]):.3e}")


if __name__ == "__main__":
    main()
