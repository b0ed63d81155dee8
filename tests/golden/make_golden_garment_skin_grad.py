#!/usr/bin/env python
"""Generate tests/golden/garment_skin_grad.npz: the gradient of the reference's own `PCALBSGarmentUseSegEncoderSeg.lbs_garment_interpolation`
(modules/mesh_encoder.py:312-410) with respect to its first argument, by torch autograd, in fp32 and in float64.

Run from the repo root:  python tests/golden/make_golden_garment_skin_grad.py     (its own process, as make_golden_refine.py, whose loader of the
reference and whose stand-ins it uses).  Needs G4D_REFERENCE_DIR; needs no GPU.  Only DATA is written: gradients, the neighbour lists, the joint
transforms the reference computed, and the reference's own fp32-vs-float64 error; the inputs are regenerated from seeds
(tests/garment_skin_grad_twin.py: golden_case).

Stand-ins beyond make_golden_refine.py's:
  * `chamferdist.knn_points` -> idx from the oracle (oracle/refine_oracle.knn_points: squared L2, ascending, lowest index first on ties), a
    constant; dists RECOMPUTED in torch from the gathered points, ((p1[:, :, None] - p2[idx]) ** 2).sum(-1), so that they carry a graph to p1.
    chamferdist's own backward (its CUDA kernel's gradient of the distances) therefore remains unpinned; what is pinned is everything the
    reference builds on top of the distances.
  * the float64 run sets torch's default dtype to float64 (the method creates its pose and ones tensors in the default dtype) and converts the
    smoothing operator to a float64 sparse tensor from the scipy matrix (gcn_utils rounds its values to float32 on the way).
Cases: K = 3 and K = 256; the second clip's pose is all zero; no garment vertex coincides with a body vertex (asserted: every distance > 0)."""
import collections
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_golden_refine as MR  # noqa: E402
import garment_skin_grad_twin as GT  # noqa: E402
from oracle import refine_oracle as RO  # noqa: E402


def main():
    torch.set_num_threads(1)
    MR.K.set_contraction("nvcc")
    me = MR.load_reference()
    KNN = collections.namedtuple("KNN", "dists idx knn")

    def knn_points(p1, p2, K=1, **kw):
        _, i = RO.knn_points(MR.N(p1).astype(np.float32), MR.N(p2).astype(np.float32), K)
        idx = MR.T(i.astype(np.int64))
        nb = p2[torch.arange(p2.shape[0])[:, None, None], idx]
        return KNN(dists=((p1[:, :, None] - nb) ** 2).sum(-1), idx=idx, knn=None)
    me.knn_points = knn_points
    case = GT.golden_case()
    faces = case["body"]["faces"]
    out = {}
    rigid = me.batch_rigid_transform
    sparse = me.gcn_utils.sparse_mx_to_torch_sparse_tensor

    def sparse64(m):
        m = m.tocoo()
        return torch.sparse_coo_tensor(MR.T(np.vstack((m.row, m.col)).astype(np.int64)), MR.T(m.data.astype(np.float64)), m.shape)
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        torch.set_default_dtype(dtype)
        seen = []
        me.batch_rigid_transform = lambda *a, **k: (lambda r: (seen.append(r[1]), r)[1])(rigid(*a, **{**k, "dtype": dtype}))
        me.gcn_utils.sparse_mx_to_torch_sparse_tensor = sparse if dtype == torch.float32 else sparse64
        model = MR.build_model(me, case).to(dtype)
        cast = lambda a: MR.T(a).to(dtype)
        batch = {k: cast(v) for k, v in case["batch"].items()}
        body_model = types.SimpleNamespace(parents=MR.T(case["body"]["parents"]), faces=faces, J_regressor=cast(case["body"]["J_regressor"]))
        for Kn in (3, 256):
            del seen[:]
            x = cast(case["tpose_garment"]).requires_grad_(True)
            posed, nn1, stage1 = model.lbs_garment_interpolation(
                x, batch["Tpose_smpl_vertices_torch"], batch["Tpose_smpl_root_joints_torch"], batch["zeropose_smpl_vertices_torch"], body_model,
                batch["pose_torch"], batch["T_J_regressor"], batch["T_lbs_weights"], K=Kn)
            assert posed.grad_fn is not None and stage1.grad_fn is not None
            for name, loss in (("posed", (posed * cast(case["dy"])).sum()), ("both", (posed * cast(case["dy"])).sum() + (stage1 * cast(case["ds"])).sum())):
                x.grad = None
                loss.backward(retain_graph=True)
                assert torch.isfinite(x.grad).all()
                out[f"k{Kn}_{name}_dx{tag}"] = MR.N(x.grad)
            if tag == "64":
                g = MR.N(x) + case["batch"]["Tpose_smpl_root_joints_torch"].reshape(-1, 1, 3)
                d, i = RO.knn_points(g.astype(np.float32), case["batch"]["Tpose_smpl_vertices_torch"].reshape(case["nbatch"], -1, 3), Kn)
                assert (d > 0).all()
                out[f"k{Kn}_idx"] = i.astype(np.int16)
                out["inv_A64"], out["A64"] = MR.N(seen[0]), MR.N(seen[1])
    torch.set_default_dtype(torch.float32)
    for Kn in (3, 256):
        for name in ("posed", "both"):
            out[f"k{Kn}_{name}_eref"] = np.abs(out[f"k{Kn}_{name}_dx32"].astype(np.float64) - out[f"k{Kn}_{name}_dx64"]).max()
            print(f"K={Kn} {name}: max |grad| {np.abs(out[f'k{Kn}_{name}_dx64']).max():.3e}, reference fp32 vs float64 {out[f'k{Kn}_{name}_eref']:.3e}")
    assert (case["batch"]["pose_torch"][1] == 0).all()
    path = os.path.join(MR.OUT, "garment_skin_grad.npz")
    np.savez_compressed(path, **out)
    print("garment_skin_grad.npz", len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
