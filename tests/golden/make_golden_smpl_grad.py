"""Regenerates tests/golden/smpl_grad.npz: the gradients of the REFERENCE's own smplx.lbs.lbs (smplx/smplx/lbs.py:152-248) to pose and betas,
by torch autograd on the CPU, in fp32 and in float64.

Run from the repo root:  G4D_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_golden_smpl_grad.py
Needs a checkout of the reference (read-only) and no GPU; no test runs it.  Only DATA is written.

Three cases on synthetic.smpl_like_params(V=97) (J = 24, NB = 10), B = 5 frames, L = sum(verts * g_v) + sum(posed_joints * g_p) with fixed
random g_v (B,V,3), g_p (B,J,3):
  a_  axis-angle pose (pose2rot=True), synthetic.smpl_like_pose
  b_  rotation matrices (pose2rot=False): Rodrigues of that pose plus 0.01 * N(0,1) per entry (not orthonormal: d pose is dR, entry by entry)
  c_  axis-angle pose whose joints 0, 3, 7, 23 are all-zero in every frame and whose frame 2 is all-zero as a whole
Stored per case: betas, pose, g_v, g_p, the fp32 run's verts / joints / d_pose / d_betas, and per gradient eref_<key> = max |fp32 - float64| of
the reference itself and max64_<key> = max |float64|.  The model constants are stored once (P_<name>)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = os.environ.get("G4D_REFERENCE_DIR") or sys.exit("set G4D_REFERENCE_DIR to a checkout of the reference")
OUT = os.environ.get("G4D_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(REF, "smplx"))
from smplx.lbs import batch_rodrigues, lbs  # noqa: E402  (the reference's)

from garment4d_amd import synthetic as syn  # noqa: E402

V, J, NB, B = 97, 24, 10, 5


def run(P, betas, pose, gv, gp, pose2rot, dtype):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    b, p = t(betas).requires_grad_(True), t(pose).requires_grad_(True)
    verts, joints = lbs(b, p, t(P["v_template"]), t(P["shapedirs"]), t(P["posedirs"]), t(P["J_regressor"]), torch.from_numpy(P["parents"]).long(),
                        t(P["lbs_weights"]), pose2rot=pose2rot)
    ((verts * t(gv)).sum() + (joints * t(gp)).sum()).backward()
    return dict(verts=verts.detach().numpy(), joints=joints.detach().numpy(), d_pose=p.grad.numpy(), d_betas=b.grad.numpy())


def main():
    P = syn.smpl_like_params(V=V, J=J, num_betas=NB, seed=11)
    betas, pose = syn.smpl_like_pose(B, J=J, num_betas=NB, seed=12)
    rng = np.random.default_rng(13)
    gv, gp = rng.standard_normal((B, V, 3)).astype(np.float32), rng.standard_normal((B, J, 3)).astype(np.float32)
    rot = batch_rodrigues(torch.from_numpy(pose).reshape(-1, 3)).reshape(B, J, 3, 3).numpy()
    rot = (rot + 0.01 * rng.standard_normal(rot.shape)).astype(np.float32)
    zpose = pose.reshape(B, J, 3).copy()
    zpose[:, [0, 3, 7, 23]] = 0
    zpose[2] = 0
    out = {"P_" + k: v for k, v in P.items()}
    for name, p, p2r in (("a", pose, True), ("b", rot, False), ("c", zpose.reshape(B, J * 3), True)):
        r32, r64 = run(P, betas, p, gv, gp, p2r, torch.float32), run(P, betas, p, gv, gp, p2r, torch.float64)
        out.update({f"{name}_betas": betas, f"{name}_pose": p, f"{name}_g_v": gv, f"{name}_g_p": gp, f"{name}_pose2rot": np.array(p2r)})
        for k in ("verts", "joints", "d_pose", "d_betas"):
            out[f"{name}_{k}"] = r32[k].astype(np.float32)
            out[f"{name}_{k}64"] = r64[k]
            out[f"{name}_eref_{k}"] = np.array(np.abs(r32[k].astype(np.float64) - r64[k]).max())
            out[f"{name}_max64_{k}"] = np.array(np.abs(r64[k]).max())
        assert np.isfinite(r32["d_pose"]).all() and np.isfinite(r64["d_pose"]).all()
        print(name, {k: (float(out[f"{name}_eref_{k}"]), float(out[f"{name}_max64_{k}"])) for k in ("d_pose", "d_betas")})
    for name in ("a", "b", "c"):          # the float64 vertices are not needed by any test
        del out[f"{name}_verts64"], out[f"{name}_joints64"]
    np.savez_compressed(os.path.join(OUT, "smpl_grad.npz"), **out)


if __name__ == "__main__":
    main()
