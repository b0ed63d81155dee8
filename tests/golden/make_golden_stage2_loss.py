#!/usr/bin/env python
"""Generate tests/golden/stage2_loss.npz: the REFERENCE's own `temporal_loss_PCA_LBS` (smplx/loss/temporal_loss.py:147-201) and torch's
autograd of its `total_loss`, on the CPU, in fp32 and on a float64 copy of the same inputs.

Run from the repo root:  G4D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_stage2_loss.py
(its own process; G4D_GOLDEN_OUT=<dir> writes elsewhere, to compare).  Needs no GPU.  Only DATA is written.

Same stand-ins as make_golden_refine.py (whose loader this script imports; `chamferdist.knn_points` is oracle/refine_oracle.knn_points: squared
L2, lowest index on ties).  After load_reference() `smplx.loss` is registered as a package (its directory has no __init__.py that could run)
and `utils.config.cfg.LOSS` is filled with cfgs/tshirt.yaml's four lambdas (20 / 10 / 100 / 5).  The vertex-face incidence that
calc_interpenetration_loss would take from openmesh is preset from the face list, as in make_golden_refine.py.
Inputs: garment4d_amd/synthetic.py:stage2_loss_case; lap_adj = I - D^-1 adj_old as the model builds it, fp32 entries (promoted exactly for
the float64 run, so that both precisions apply the same operator).

Stored: every scalar of loss_dict (fp32 run) with eref_<key> = |fp32 - float64| and max64_<key>; lbs_garment_msre_list; grad0..2 = d total_loss
/ d round (fp32) with eref_grad<r>, max64_grad<r>; `decisions` = [penetration signs, nearest indices] that differ between the two precisions
(asserted 0, like the 20-80 % penetrating share per round); the float64 scalars themselves (f64_<key>) for the twin's CPU test -- the float64
gradients are not stored (file size): the twin is held to the fp32 ones within eref; checksum."""
import importlib
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

from garment4d_amd import gcn  # noqa: E402
from garment4d_amd import synthetic as syn  # noqa: E402
import stage2_loss_twin as TW  # noqa: E402

T_, N_ = MG.T, MG.N
SCALARS = ("lbs_garment_msre", "only_lbs_garment_msre", "lbs_garment_l2_loss", "lbs_garment_lap_loss", "lbs_interpenetration_loss",
           "temporal_constraint_loss", "acceleration_error", "only_lbs_acceleration_error", "total_loss")


def run(tl, case, lap, dt):
    faces = case["body"]["faces"]
    tl.vf_vid = T_(np.concatenate([faces[:, c] for c in range(3)]).astype(np.int64))
    tl.vf_fid = T_(np.concatenate([np.arange(faces.shape[0])] * 3).astype(np.int64))
    rec = dict(sign=[], idx=[])
    saved = (tl.F.relu, tl.knn_points)

    def relu(x, *a, **k):
        rec["sign"].append(N_(x > 0).copy())
        return saved[0](x, *a, **k)

    def knn(p1, p2, *a, **k):
        out = saved[1](p1, p2, *a, **k)
        rec["idx"].append(N_(out.idx).copy())
        return out
    tl.F.relu, tl.knn_points = relu, knn
    try:
        rounds = [T_(p).to(dt).requires_grad_(True) for p in case["rounds"]]
        od = dict(iter_regressed_lbs_garment_v=rounds, lbs_pred_garment_v=T_(case["lbs_pred_garment_v"]).to(dt), lap_adj=lap.to(dt))
        inputs = {k: T_(v).to(dt) for k, v in case["inputs"].items()}
        inputs["garment_template_vertices"] = torch.zeros(case["nbatch"], case["Vg"], 3, dtype=dt)   # read at :172, its result never used
        body_model = types.SimpleNamespace(faces=faces)
        ld = tl.temporal_loss_PCA_LBS(od, inputs, body_model, types.SimpleNamespace())
        ld["total_loss"].backward()
    finally:
        tl.F.relu, tl.knn_points = saved
    return {k: N_(v).copy() for k, v in ld.items()}, [N_(p.grad).copy() for p in rounds], rec


def main():
    torch.set_num_threads(1)
    MG.load_reference()
    MG._pkg("smplx.loss", os.path.join(MG.REF, "smplx", "loss"))
    cfg = sys.modules["utils.config"].cfg
    cfg.LOSS = types.SimpleNamespace(**dict(zip(("LBS_GARMENT_L2_LOSS_LAMBDA", "LBS_GARMENT_LAP_LOSS_LAMBDA", "LBS_INTERPENETRATION_LOSS_LAMBDA",
                                                 "TEMPORAL_CONSTRAINT_LOSS_LAMBDA"), TW.LAMBDAS)))
    tl = importlib.import_module("smplx.loss.temporal_loss")
    case = syn.stage2_loss_case()
    lap = gcn.sparse_mx_to_torch_sparse_tensor(TW.laplacian_from_faces(case["template_faces"], case["Vg"]))
    d32, g32, rec32 = run(tl, case, lap, torch.float32)
    d64, g64, rec64 = run(tl, case, lap, torch.float64)
    out = {}
    for k in SCALARS:
        assert d32[k].dtype == np.float32 and d64[k].dtype == np.float64 and d32[k].shape == (), k
        out[k], out[f"f64_{k}"] = d32[k], d64[k]
        out[f"eref_{k}"] = np.float64(abs(float(d32[k]) - float(d64[k])))
        out[f"max64_{k}"] = np.float64(abs(float(d64[k])))
    out["lbs_garment_msre_list"], out["f64_lbs_garment_msre_list"] = d32["lbs_garment_msre_list"], d64["lbs_garment_msre_list"]
    out["eref_lbs_garment_msre_list"] = np.float64(np.abs(d32["lbs_garment_msre_list"].astype(np.float64) - d64["lbs_garment_msre_list"]).max())
    for r in range(3):
        assert g32[r].dtype == np.float32 and g64[r].dtype == np.float64
        out[f"grad{r}"] = g32[r]
        out[f"eref_grad{r}"] = np.float64(np.abs(g32[r].astype(np.float64) - g64[r]).max())
        out[f"max64_grad{r}"] = np.float64(np.abs(g64[r]).max())
    assert len(rec32["sign"]) == len(rec64["sign"]) == 3 and len(rec32["idx"]) == len(rec64["idx"]) == 3
    out["decisions"] = np.array([sum(int((a != b).sum()) for a, b in zip(rec32[k], rec64[k])) for k in ("sign", "idx")], dtype=np.int64)
    out["penetrating_share"] = np.array([float(s.mean()) for s in rec32["sign"]])
    assert (out["decisions"] == 0).all(), out["decisions"]
    assert ((out["penetrating_share"] >= 0.2) & (out["penetrating_share"] <= 0.8)).all(), out["penetrating_share"]
    out["checksum"] = syn.stage2_loss_checksum(case)
    path = os.path.join(OUT, "stage2_loss.npz")
    np.savez_compressed(path, **out)
    print("stage2_loss.npz", len(out), "arrays", os.path.getsize(path), "bytes; penetrating", out["penetrating_share"])
    for k in SCALARS:
        print(f"  {k}: {float(out[k]):.9g}  eref {float(out['eref_' + k]):.3e}")
    for r in range(3):
        print(f"  grad{r}: eref {float(out['eref_grad%d' % r]):.3e}  max64 {float(out['max64_grad%d' % r]):.3e}")


if __name__ == "__main__":
    main()
