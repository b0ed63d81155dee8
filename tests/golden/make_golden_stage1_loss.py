#!/usr/bin/env python
"""Generate tests/golden/stage1_loss.npz: the REFERENCE's own `temporal_loss_PCA` (smplx/loss/temporal_loss.py:60-119, with the one-time
cotangent Laplacian of smplx/loss/laplacian.py) and torch's autograd of its `total_loss`, on the CPU, in fp32 and on a float64 copy of the
same inputs.

Run from the repo root:  G4D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_stage1_loss.py
(its own process; G4D_GOLDEN_OUT=<dir> writes elsewhere, to compare).  Needs no GPU.  Only DATA is written.

Same stand-ins as make_golden_refine.py (whose loader this script imports: `Tensor.cuda` as the identity, `chamferdist.knn_points` =
oracle/refine_oracle.knn_points, squared L2, lowest index on ties).  After load_reference() `smplx.loss` is registered as a package and
`utils.config.cfg` is filled with cfgs/tshirt.yaml's five lambdas (0.05 / 0.001 / 40 / 50 / 1), NETWORK.NPOINTS and GARMENT.PCADIM.  The
vertex-face incidence that calc_interpenetration_loss would take from openmesh is preset from the face list, as in make_golden_refine.py.
Two more stand-ins, neither touching the reference's files:
  * temporal_loss.py:71 reshapes the T-pose body to a hard-coded 6890 vertices; the synthetic body has 700.  The input is handed over in a
    wrapper whose reshape(b, 6890, 3) is reshape(b, -1, 3).
  * FOR THE FLOAT64 RUN ONLY the run must be float64 throughout, or e_ref = |ref32 - ref64| would be too small for the Laplacian term:
    laplacian.py's `convert_as(torch.Tensor(Lx), V)` rounds L x through float32 (torch.Tensor(...) is a float32 constructor), and so do the
    `.float()` calls on the curvature norms (:457, :466).  For that run the module's `convert_as` returns its argument, the module's name
    `torch` resolves to a forwarding object whose `Tensor(a)` keeps the array's dtype, and `Tensor.float` is the identity.
In both runs the same forwarding object records the sign of n_i - c_i that `torch.abs` sees in OnetimeLaplacianLoss.__call__.
Inputs: garment4d_amd/synthetic.py:stage1_loss_case.

Stored: every scalar of loss_dict (fp32 run) with f64_<key>, eref_<key> = |fp32 - float64| and max64_<key>; grad_logits / grad_coeff /
grad_pred = d total_loss / d (sem_logits, garment_PCA_coeff, tpose_garment) in fp32 with f64_grad_*, eref_grad_*, max64_grad_*; `decisions` =
[penetration signs, nearest indices, signs of n_i - c_i] that differ between the two precisions (asserted 0); the penetrating share (asserted
within 20-80 %); a second pair of runs with args.only_seg (os_<key>, f64_os_<key>, eref_os_<key>, os_keys); checksum."""
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

from garment4d_amd import synthetic as syn  # noqa: E402
import stage1_loss_twin as TW  # noqa: E402

T_, N_ = MG.T, MG.N
LEAVES = (("logits", "sem_logits"), ("coeff", "garment_PCA_coeff"), ("pred", "tpose_garment"))


class AnyVertexCount:
    """Stands in for inputs['Tpose_smpl_vertices_torch']: .cuda() is the identity, .reshape(b, 6890, 3) takes the vertex count from the data."""
    def __init__(self, t):
        self.t = t

    def cuda(self):
        return self

    def reshape(self, b, _v, c):
        return self.t.reshape(b, -1, c)


class TorchShim:
    """What smplx.loss.laplacian sees under the name `torch`: everything forwarded; abs() records the sign of its argument; with keep_dtype,
    Tensor(a) keeps the array's dtype."""
    def __init__(self, rec, keep_dtype):
        self._rec, self._keep = rec, keep_dtype

    def __getattr__(self, name):
        return getattr(torch, name)

    def abs(self, x):
        self._rec.append(np.sign(N_(x)).copy())
        return torch.abs(x)

    def Tensor(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)) if self._keep else torch.Tensor(a)


def run(tl, lap, case, dt, only_seg):
    faces = case["body"]["faces"]
    tl.vf_vid = T_(np.concatenate([faces[:, c] for c in range(3)]).astype(np.int64))
    tl.vf_fid = T_(np.concatenate([np.arange(faces.shape[0])] * 3).astype(np.int64))
    rec = dict(sign=[], idx=[], lap=[])
    f64 = dt == torch.float64
    saved = (tl.F.relu, tl.knn_points, lap.torch, lap.convert_as, torch.Tensor.float)

    def relu(x, *a, **k):
        rec["sign"].append(N_(x > 0).copy())
        return saved[0](x, *a, **k)

    def knn(p1, p2, *a, **k):
        out = saved[1](p1, p2, *a, **k)
        rec["idx"].append(N_(out.idx).copy())
        return out
    tl.F.relu, tl.knn_points, lap.torch = relu, knn, TorchShim(rec["lap"], f64)
    if f64:
        lap.convert_as = lambda src, trg: src
        torch.Tensor.float = lambda self: self
    try:
        od = {k: T_(v).to(dt).requires_grad_(True) for k, v in case["output"].items() if k != "garment_f_3"}
        od["garment_f_3"] = case["output"]["garment_f_3"]
        inputs = {k: (T_(v).to(dt) if v.dtype == np.float32 else T_(v)) for k, v in case["inputs"].items()}
        inputs["smpl_vertices_torch"] = torch.zeros(case["nbatch"], case["T"], 1, 3, dtype=dt)       # read at :67-68, their result never used
        inputs["smpl_root_joints_torch"] = torch.zeros(case["nbatch"], case["T"], 3, dtype=dt)
        inputs["Tpose_smpl_vertices_torch"] = AnyVertexCount(inputs["Tpose_smpl_vertices_torch"])
        args = types.SimpleNamespace(only_seg=only_seg, batch_size=case["pad_batch"])
        ld = tl.temporal_loss_PCA(od, inputs, types.SimpleNamespace(faces=faces), args)
        ld["total_loss"].backward()
    finally:
        tl.F.relu, tl.knn_points, lap.torch, lap.convert_as, torch.Tensor.float = saved
    grads = {s: (None if od[k].grad is None else N_(od[k].grad).copy()) for s, k in LEAVES}
    return {k: N_(v).copy() for k, v in ld.items()}, grads, rec


def main():
    torch.set_num_threads(1)
    MG.load_reference()
    MG._pkg("smplx.loss", os.path.join(MG.REF, "smplx", "loss"))
    case = syn.stage1_loss_case()
    cfg = sys.modules["utils.config"].cfg
    cfg.LOSS = types.SimpleNamespace(**dict(zip(("SEM_SEG_LOSS_LAMBDA", "GARMENT_PCA_COEFF_L2_LAMBDA", "GARMENT_L2_LOSS_LAMBDA",
                                                 "INTERPENETRATION_LOSS_LAMBDA", "GARMENT_LAP_LOSS_LAMBDA"), TW.LAMBDAS)))
    cfg.NETWORK = types.SimpleNamespace(NPOINTS=case["N"])
    cfg.GARMENT = types.SimpleNamespace(PCADIM=case["P"])
    tl = importlib.import_module("smplx.loss.temporal_loss")
    lap = importlib.import_module("smplx.loss.laplacian")
    d32, g32, rec32 = run(tl, lap, case, torch.float32, False)
    d64, g64, rec64 = run(tl, lap, case, torch.float64, False)
    assert set(d32) == set(TW.KEYS) == set(d64)
    out = {}
    for k in TW.KEYS:
        assert d32[k].dtype == np.float32 and d64[k].dtype == np.float64 and d32[k].shape == (), (k, d32[k].dtype, d64[k].dtype)
        out[k], out[f"f64_{k}"] = d32[k], d64[k]
        out[f"eref_{k}"] = np.float64(abs(float(d32[k]) - float(d64[k])))
        out[f"max64_{k}"] = np.float64(abs(float(d64[k])))
    for s, _ in LEAVES:
        assert g32[s].dtype == np.float32 and g64[s].dtype == np.float64
        out[f"grad_{s}"], out[f"f64_grad_{s}"] = g32[s], g64[s]
        out[f"eref_grad_{s}"] = np.float64(np.abs(g32[s].astype(np.float64) - g64[s]).max())
        out[f"max64_grad_{s}"] = np.float64(np.abs(g64[s]).max())
    assert len(rec32["sign"]) == len(rec64["sign"]) == 1 and len(rec32["idx"]) == len(rec64["idx"]) == 1 and len(rec32["lap"]) == len(rec64["lap"]) == 1
    out["decisions"] = np.array([sum(int((a != b).sum()) for a, b in zip(rec32[k], rec64[k])) for k in ("sign", "idx", "lap")], dtype=np.int64)
    out["penetrating_share"] = np.array([float(s.mean()) for s in rec32["sign"]])
    assert (out["decisions"] == 0).all(), out["decisions"]
    assert ((out["penetrating_share"] >= 0.2) & (out["penetrating_share"] <= 0.8)).all(), out["penetrating_share"]
    o32, og32, _ = run(tl, lap, case, torch.float32, True)
    o64, og64, _ = run(tl, lap, case, torch.float64, True)
    assert set(o32) == {"sem_seg_loss", "total_loss"} == set(o64) and og32["coeff"] is None and og32["pred"] is None
    out["os_keys"] = np.array(sorted(o32))
    for k in o32:
        out[f"os_{k}"], out[f"f64_os_{k}"] = o32[k], o64[k]
        out[f"eref_os_{k}"] = np.float64(abs(float(o32[k]) - float(o64[k])))
    out["os_grad_logits"], out["f64_os_grad_logits"] = og32["logits"], og64["logits"]
    out["eref_os_grad_logits"] = np.float64(np.abs(og32["logits"].astype(np.float64) - og64["logits"]).max())
    out["checksum"] = syn.stage1_loss_checksum(case)
    path = os.path.join(OUT, "stage1_loss.npz")
    np.savez_compressed(path, **out)
    print("stage1_loss.npz", len(out), "arrays", os.path.getsize(path), "bytes; penetrating", out["penetrating_share"])
    for k in TW.KEYS:
        print(f"  {k}: {float(out[k]):.9g}  f64 {float(out['f64_' + k]):.12g}  eref {float(out['eref_' + k]):.3e}")
    for s, _ in LEAVES:
        print(f"  grad_{s}: eref {float(out['eref_grad_' + s]):.3e}  max64 {float(out['max64_grad_' + s]):.3e}")


if __name__ == "__main__":
    main()
