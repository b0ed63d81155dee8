"""float64 twin of the MGN training route (garment4d_amd/csrc/mgn_skin_grad.hip, mesh_encoder._LinearFn; modules/mesh_encoder.py:529-614 in the
reference), shared by tests/test_mgn_grad_cpu.py (which ties it to the reference's own run through tests/golden/mgn_grad.npz) and
tests/test_mgn_grad_gpu.py (which holds the kernels to it).  Not a test module.

Two parts.  numpy only: the two blends at a FIXED nearest index, s = M_inv [q; 1], p = M [s; 1], and their adjoint
d_garment = M_inv3^T (M3^T d_posed + d_stage1) (M3 = the 3x3 part; the translation columns and the root add drop out).  torch float64: displacement
MLP -> * 0.05 / NaN -> 0 -> the skinning at the fixed index -> the stage-2 loss twin (tests/stage2_loss_twin.py, whose analytic gradient enters
the torch graph as the cotangent of the prediction).

Error bound of g4d_mgn_skin_grad_f32, first order, u = 2^-24, from the kernel's documented arithmetic (include/g4d.h); nothing is measured:
  an entry of M or M_inv   acc = fma(w_j, T_j, acc), j = 0..J-1 from 0: J roundings, each of a partial sum no larger than sum_j |w_j| |T_j|
                           -> J u |M|, with |M| formed as sum_j |w_j| |T_j|
  t[k]                     fma(M[2][k], d2, fma(M[1][k], d1, fma(M[0][k], d0, d_stage1[k]))): 3 roundings of partial sums, on top of the entries'
                           errors -> (J + 3) u tb[k],   tb = |M3|^T |d_posed| + |d_stage1|
  d_garment[k]             fma(Mi[2][k], t2, fma(Mi[1][k], t1, Mi[0][k] t0)): 3 roundings, the entries' errors J u, and the error of t carried
                           through |M_inv3|^T -> (J + 3) u |M_inv3|^T tb + (J + 3) u |M_inv3|^T tb
so the constant is 2 J + 6 -- NOT the J + 8 first proposed for this bound: that counts one blend's J roundings, but the result is a product of
two blended matrices and each carries its own J.  bound = (2 J + 6) u |M_inv3|^T (|M3|^T |d_posed| + |d_stage1|) per output component.

The forward's rounding of `posed`, for the adjoint identity <posed(q + delta) - posed(q), g> = <delta, grad(g)>: terms = |M3| (|M_inv3| |q| + |t_inv|) +
|t|, the sum of absolute values of everything that is added up to form one component of posed; a launch is held to (J + 8) u terms and the
difference of two launches, paired with g, to 2 (J + 8) u sum(terms |g|).

Linear nodes (existing kernels): the project's rule for a k-term fp32 contraction in any order, (k + 2) u sum |terms| (gcn_grad_twin.sum_bound):
k = rows for dW and db, k = Cout for dX."""
import os

import numpy as np

import stage2_loss_twin as TW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
LAYERS = (0, 2, 4)


def load():
    return np.load(os.path.join(GOLDEN, "mgn_grad.npz"))


def golden_inputs():
    """(case, targets, displacement state dict) of tests/golden/mgn_grad.npz, regenerated from the seeds (+ `fwd_posed` of mgn.npz)."""
    from garment4d_amd import synthetic as syn
    case = syn.mgn_golden_case()
    posed = np.load(os.path.join(GOLDEN, "mgn.npz"))["fwd_posed"]
    return case, syn.mgn_grad_targets(case, posed), syn.mgn_displacement_state_dict(case["Vg"], seed=case["seed"] + 100)


# ------------------------------------------------------------------------------------------------ the joint transforms, float64
def rodrigues64(r):
    """smplx/transfer_model/utils/pose_utils.py:62-99: angle = |r + 1e-8|, R = I + sin K + (1 - cos) K K."""
    r = np.asarray(r, np.float64)
    angle = np.linalg.norm(r + 1e-8, axis=1, keepdims=True)
    d = r / angle
    z = np.zeros(len(r))
    K = np.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).reshape(-1, 3, 3)
    s, c = np.sin(angle)[:, :, None], np.cos(angle)[:, :, None]
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K)


def rigid_transform64(rot, joints, parents):
    """smplx/smplx/lbs.py:362-419 -> the relative transforms A (F,J,4,4)."""
    rot, joints = np.asarray(rot, np.float64), np.asarray(joints, np.float64)
    F_, J = joints.shape[:2]
    rel = joints.copy()
    rel[:, 1:] -= joints[:, parents[1:]]
    tm = np.zeros((F_, J, 4, 4))
    tm[..., :3, :3], tm[..., :3, 3], tm[..., 3, 3] = rot, rel, 1.0
    chain = [tm[:, 0]]
    for i in range(1, J):
        chain.append(chain[int(parents[i])] @ tm[:, i])
    tr = np.stack(chain, 1)
    tj = tr @ np.concatenate([joints, np.zeros((F_, J, 1))], -1)[..., None]
    out = tr.copy()
    out[..., 3] -= tj[..., 0]
    return out


def transforms64(batch, parents):
    """(inv_A, A) (F,J,4,4) of lbs_garment_MGN (modules/mesh_encoder.py:543-572) from the batch's numpy arrays."""
    pose = np.asarray(batch["pose_torch"], np.float64)
    nbatch, T = pose.shape[:2]
    F_ = nbatch * T
    Jreg = np.asarray(batch["T_J_regressor"], np.float64).reshape(F_, 24, -1)
    V = Jreg.shape[-1]
    tpose = np.repeat(np.asarray(batch["Tpose_smpl_vertices_torch"], np.float64).reshape(nbatch, 1, V, 3), T, 1).reshape(F_, V, 3)
    inv_pose = np.zeros((F_, 24, 3))
    inv_pose[:, 0, 0], inv_pose[:, 1, 1], inv_pose[:, 2, 1] = -np.pi / 2, 0.15, -0.15
    inv_A = rigid_transform64(rodrigues64(inv_pose.reshape(-1, 3)).reshape(F_, 24, 3, 3), np.einsum("fjv,fvk->fjk", Jreg, tpose), parents)
    zero = np.asarray(batch["zeropose_smpl_vertices_torch"], np.float64).reshape(F_, V, 3)
    A = rigid_transform64(rodrigues64(pose.reshape(-1, 3)).reshape(F_, 24, 3, 3), np.einsum("fjv,fvk->fjk", Jreg, zero), parents)
    return inv_A, A


# ------------------------------------------------------------------------------------------------ the blends and their adjoint, numpy
def blends64(idx, W, inv_A, A):
    """(M_inv, M, |M_inv|, |M|) (F,Vg,4,4) at the nearest vertices idx (F,Vg); |M| = sum_j |w_j| |T_j|."""
    idx = np.asarray(idx, np.int64)
    W, inv_A, A = (np.asarray(a, np.float64) for a in (W, inv_A, A))
    w = W[np.arange(W.shape[0])[:, None], idx]                           # (F,Vg,J)
    e = lambda w_, t: np.einsum("fgj,fjab->fgab", w_, t)
    return e(w, inv_A), e(w, A), e(np.abs(w), np.abs(inv_A)), e(np.abs(w), np.abs(A))


def skin64(q, idx, W, inv_A, A):
    """(stage 1, posed, terms) for the queries q (F,Vg,3) = garment + root; terms: see the module docstring."""
    Mi, M, aMi, aM = blends64(idx, W, inv_A, A)
    q = np.asarray(q, np.float64)
    mv = lambda m, x: np.einsum("fgab,fgb->fga", m[..., :3, :3], x) + m[..., :3, 3]
    s = mv(Mi, q)
    p = mv(M, s)
    return s, p, mv(aM, mv(aMi, np.abs(q)))


def skin_adjoint64(idx, W, inv_A, A, d_posed, d_stage1=None):
    """(d_garment (F,Vg,3), bound (F,Vg,3)): M_inv3^T (M3^T d_posed + d_stage1) and the derived bound of the kernel."""
    Mi, M, aMi, aM = blends64(idx, W, inv_A, A)
    J = np.asarray(W).shape[-1]
    dp = np.asarray(d_posed, np.float64)
    ds = np.zeros_like(dp) if d_stage1 is None else np.asarray(d_stage1, np.float64)
    tv = lambda m, x: np.einsum("fgab,fga->fgb", m[..., :3, :3], x)
    grad = tv(Mi, tv(M, dp) + ds)
    return grad, (2 * J + 6) * U * tv(aMi, tv(aM, np.abs(dp)) + np.abs(ds))


def reference_blend_torch(garment, root, idx, W, inv_A, A, T):
    """The reference's own formulation (:553-583) on torch tensors: blend ALL body vertices' transforms with a matmul, gather the nearest one's,
    apply to homogeneous coordinates.  garment (F,Vg,3) (may require grad), root (clips,3) -> (stage 1, posed)."""
    import torch
    F_, Vg, _ = garment.shape
    J = W.shape[-1]
    q = garment + root.reshape(-1, 1, 1, 3).repeat(1, T, 1, 1).reshape(F_, 1, 3)
    rep = idx.reshape(F_, Vg, 1, 1).repeat(1, 1, 4, 4)
    ones = torch.ones((F_, Vg, 1), dtype=garment.dtype)
    inv_T = torch.gather(torch.matmul(W, inv_A.reshape(F_, J, 16)).view(F_, -1, 4, 4), 1, rep)
    s = torch.matmul(inv_T, torch.cat([q, ones], 2).unsqueeze(-1))[:, :, :3, 0]
    nn_T = torch.gather(torch.matmul(W, A.reshape(F_, J, 16)).view(F_, -1, 4, 4), 1, rep)
    return s, torch.matmul(nn_T, torch.cat([s, ones], 2).unsqueeze(-1))[:, :, :3, 0]


# ------------------------------------------------------------------------------------------------ the training step, torch float64
class _SkinFn64:
    """Built lazily (torch import): an autograd node on skin64 / skin_adjoint64, so the numpy adjoint is what the twin differentiates with."""
    fn = None

    @classmethod
    def get(cls):
        if cls.fn is None:
            import torch

            class Fn(torch.autograd.Function):
                @staticmethod
                def forward(ctx, q, consts):
                    ctx.consts = consts
                    s, p, _ = skin64(q.detach().numpy(), *consts)
                    return torch.from_numpy(s), torch.from_numpy(p)

                @staticmethod
                def backward(ctx, ds, dp):
                    return torch.from_numpy(skin_adjoint64(*ctx.consts, dp.numpy(), ds.numpy())[0]), None
            cls.fn = Fn
        return cls.fn


def displacement_mlp64(sd, summary):
    """The three Linear layers (+ ReLU on the first two) on float64 leaves: (leaves {name: tensor}, pre-activations [3], output (F, 3 Vg))."""
    import torch
    leaves = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in sd.items()}
    h = torch.from_numpy(np.asarray(summary, np.float64)).reshape(-1, 512)
    pre = []
    for i in LAYERS:
        h = h @ leaves[f"displacement_encoder.{i}.weight"].t() + leaves[f"displacement_encoder.{i}.bias"]
        pre.append(h)
        if i != LAYERS[-1]:
            h = torch.relu(h)
    return leaves, pre, h


def train_step64(case, targets, sd, idx=None, weights=TW.LAMBDAS):
    """One forward + backward of the MGN training route in float64.  idx: the skinning's nearest index to hold fixed (default: this module's own
    float64 search).  Returns dict(loss scalars, posed, stage1, idx, d_lbs_pred, grads {name: array}, pre-activations, penetration record)."""
    import torch
    nbatch, T, Vg = case["nbatch"], case["T"], case["Vg"]
    F_ = nbatch * T
    batch = case["batch"]
    inv_A, A = transforms64(batch, np.asarray(case["body"]["parents"]))
    W = np.asarray(batch["T_lbs_weights"], np.float64).reshape(F_, -1, 24)
    leaves, pre, h = displacement_mlp64(sd, case["garment_summary"])
    d = h.reshape(F_, Vg, 3) * 0.05
    d = d.masked_fill(torch.isnan(d), 0.0)
    tg = torch.from_numpy(np.asarray(case["tpose_garment"], np.float64)).reshape(nbatch, 1, Vg, 3)
    garment = (tg + d.reshape(nbatch, T, Vg, 3)).reshape(F_, Vg, 3)
    root = np.repeat(np.asarray(batch["Tpose_smpl_root_joints_torch"], np.float64).reshape(nbatch, 1, 3), T, 1).reshape(F_, 1, 3)
    q = garment + torch.from_numpy(root)
    if idx is None:
        tp = np.repeat(np.asarray(batch["Tpose_smpl_vertices_torch"], np.float64).reshape(nbatch, 1, -1, 3), T, 1).reshape(F_, -1, 3)
        idx = TW.nearest(q.detach().numpy(), tp)[0]
    idx = np.asarray(idx, np.int64).reshape(F_, Vg)
    stage1, posed = _SkinFn64.get().apply(q, (idx, W, inv_A, A))
    # the loss: the stage-2 twin on one round, its analytic gradient as the cotangent of the prediction
    body = np.asarray(targets["smpl_vertices_torch"], np.float64).reshape(F_, -1, 3)
    gt = (np.asarray(targets["garment_torch"], np.float64) + np.asarray(targets["smpl_root_joints_torch"], np.float64)[:, :, None, :]).reshape(F_, Vg, 3)
    normals = TW.vertex_normals64(body, case["body"]["faces"])
    L = TW.laplacian_from_faces(case["template_faces"], Vg)
    p = posed.detach().numpy()
    r = TW.evaluate(p, gt, body, normals, L, nbatch, T, temporal=True)
    g, _ = TW.gradient(r, weights)
    posed.backward(torch.from_numpy(g))
    v = r["values"]
    acc = TW.acceleration_error(p, gt, nbatch, T)
    msre = v["msre"]
    scalars = {"lbs_garment_msre": msre, "only_lbs_garment_msre": msre, "lbs_garment_l2_loss": v["l2"], "lbs_garment_lap_loss": v["lap"],
               "lbs_interpenetration_loss": v["pen"], "temporal_constraint_loss": v["tmp"], "acceleration_error": acc,
               "only_lbs_acceleration_error": acc, "total_loss": TW.total([v], weights)}
    return dict(scalars=scalars, posed=p, stage1=stage1.detach().numpy(), idx=idx, d_lbs_pred=g, grads={k: t.grad.numpy() for k, t in leaves.items()},
                pre=[t.detach().numpy() for t in pre], dot=r["dot"], loss_idx=r["idx"], consts=(W, inv_A, A))


def weight_views(dw, sample):
    """The golden file's three views of a weight gradient: float64 row sums, column sums, sampled entries."""
    dw = np.asarray(dw)
    return {"rowsum": dw.astype(np.float64).sum(1), "colsum": dw.astype(np.float64).sum(0), "sample": dw.reshape(-1)[sample]}


def stored_arrays(grads, d_lbs_pred, golden):
    """{golden key: array} for a set of parameter gradients {state-dict name: array} and d total / d lbs_pred_garment_v."""
    out = {"d_lbs_pred": np.asarray(d_lbs_pred)}
    for i in LAYERS:
        out[f"db{i}"] = np.asarray(grads[f"displacement_encoder.{i}.bias"])
        for name, a in weight_views(grads[f"displacement_encoder.{i}.weight"], golden[f"sample_idx_{i}"]).items():
            out[f"dW{i}_{name}"] = a
    return out


# ------------------------------------------------------------------------------------------------ Linear nodes
def sum_bound(k, abs_sum):
    """(k + 2) u sum |terms|: a k-term fp32 contraction of exactly known factors in any order (gcn_grad_twin.sum_bound)."""
    return (k + 2) * U * abs_sum


def linear_backward64(x, w, g):
    """(db, dW (Cout,Cin), dX) and their bounds for G (rows,Cout) (already masked), X (rows,Cin), W (Cout,Cin), all float64."""
    rows, cout = g.shape
    ag, ax, aw = np.abs(g), np.abs(x), np.abs(w)
    return ((g.sum(0), sum_bound(rows, ag.sum(0))), (g.T @ x, sum_bound(rows, ag.T @ ax)), (g @ w, sum_bound(cout, ag @ aw)))
