"""numpy restatement of include/g4d_smpl.h (test infrastructure; the package never imports it): lbs() forward and its analytic adjoint in
float64, written from the formulas of the header and not via autograd, plus a plain torch restatement of the forward in the reference's op
order (smplx/smplx/lbs.py:152-248), whose fp32 autograd measures what fp32 itself costs on the inputs of a test."""
import numpy as np

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------------- the forward
def rodrigues(theta):
    """(N,3) axis-angle -> (N,3,3) by lbs.py:330-345: angle = ||t + 1e-8||, dir = t / angle, R = I + sin K + (1 - cos) K K.  Also the pieces."""
    theta = np.asarray(theta, F64)
    a = theta + 1e-8
    angle = np.sqrt((a * a).sum(1, keepdims=True))
    d = theta / angle
    K = np.zeros((len(theta), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    s, c = np.sin(angle)[:, :, None], np.cos(angle)[:, :, None]
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K), dict(a=a, angle=angle, K=K, s=s, c=c)


def constants(P):
    """smpl_like_params dict -> the prepared constants of lbs.py's fused routes, in float64."""
    V, _, NB = P["shapedirs"].shape
    blend_dirs = np.concatenate([P["shapedirs"].astype(F64).reshape(V * 3, NB).T, P["posedirs"].astype(F64)], 0)
    Jr = P["J_regressor"].astype(F64)
    return dict(blend_dirs=blend_dirs, Jt=Jr @ P["v_template"].astype(F64), Js=np.einsum("jv,vrk->jrk", Jr, P["shapedirs"].astype(F64)),
                v_template=P["v_template"].astype(F64), W=P["lbs_weights"].astype(F64), parents=np.asarray(P["parents"]).astype(np.int64))


def forward(betas, pose, P, pose2rot=True, keep=False):
    """betas (B,NB) or (1,NB), pose (B,J*3) / (B,J,3,3) -> verts (B,V,3), posed joints (B,J,3) in float64 (and every intermediate if keep)."""
    C = constants(P)
    J, V = len(C["parents"]), len(C["v_template"])
    pose = np.asarray(pose, F64)
    B = pose.shape[0]
    betas = np.broadcast_to(np.asarray(betas, F64), (B, np.shape(betas)[1]))
    NB = betas.shape[1]
    if pose2rot:
        R, rod = rodrigues(pose.reshape(B * J, 3))
        R = R.reshape(B, J, 3, 3)
    else:
        R, rod = pose.reshape(B, J, 3, 3), None
    c = np.concatenate([betas, (R[:, 1:] - np.eye(3)).reshape(B, -1)], 1)
    v_posed = C["v_template"][None] + (c @ C["blend_dirs"]).reshape(B, V, 3)
    Jr = C["Jt"][None] + np.einsum("jrk,bk->bjr", C["Js"], betas)
    GR, Gt = np.zeros((B, J, 3, 3)), np.zeros((B, J, 3))
    GR[:, 0], Gt[:, 0] = R[:, 0], Jr[:, 0]
    for j in range(1, J):
        p = C["parents"][j]
        GR[:, j] = GR[:, p] @ R[:, j]
        Gt[:, j] = np.einsum("brc,bc->br", GR[:, p], Jr[:, j] - Jr[:, p]) + Gt[:, p]
    At = Gt - np.einsum("bjrc,bjc->bjr", GR, Jr)
    TR = np.einsum("vj,bjrc->bvrc", C["W"], GR)
    Tt = np.einsum("vj,bjr->bvr", C["W"], At)
    verts = np.einsum("bvrc,bvc->bvr", TR, v_posed) + Tt
    if keep:
        return verts, Gt, dict(C=C, R=R, rod=rod, c=c, v_posed=v_posed, Jr=Jr, GR=GR, Gt=Gt, TR=TR, NB=NB, B=B, J=J, V=V, betas=betas, pose=pose)
    return verts, Gt


# ------------------------------------------------------------------------------------------------------------------------- the adjoint
def rodrigues_adjoint(theta, rod, dR):
    K, s, c, a, angle = rod["K"], rod["s"], rod["c"], rod["a"], rod["angle"]
    KK = K @ K
    ds = (dR * K).sum((1, 2))
    dc1 = (dR * KK).sum((1, 2))
    dK = s * dR + (1 - c) * (dR @ K.transpose(0, 2, 1) + K.transpose(0, 2, 1) @ dR)
    dd = np.stack([dK[:, 2, 1] - dK[:, 1, 2], dK[:, 0, 2] - dK[:, 2, 0], dK[:, 1, 0] - dK[:, 0, 1]], 1)
    dangle = ds * c[:, 0, 0] + dc1 * s[:, 0, 0] - (dd * theta).sum(1) / angle[:, 0] ** 2
    return dd / angle + dangle[:, None] * a / angle


def adjoint(betas, pose, P, d_verts, d_joints, pose2rot=True):
    """include/g4d_smpl.h's adjoint in float64: (d_betas in the shape of betas, d_pose in the shape of pose)."""
    _, _, S = forward(betas, pose, P, pose2rot, keep=True)
    C, B, J, V, NB = S["C"], S["B"], S["J"], S["V"], S["NB"]
    gv = np.zeros((B, V, 3)) if d_verts is None else np.asarray(d_verts, F64)
    gp = np.zeros((B, J, 3)) if d_joints is None else np.asarray(d_joints, F64)
    vh = np.concatenate([S["v_posed"], np.ones((B, V, 1))], 2)
    dA = np.einsum("vj,bvr,bvk->bjrk", C["W"], gv, vh)                      # (B,J,3,4)
    dvp = np.einsum("bvrc,bvr->bvc", S["TR"], gv)                            # (T^R)^T g
    dc = dvp.reshape(B, V * 3) @ C["blend_dirs"].T                           # (B,NC)
    dAR, dAt = dA[..., :3], dA[..., 3]
    dGR = dAR - np.einsum("bjr,bjc->bjrc", dAt, S["Jr"])
    dGt = dAt + gp
    dJr = -np.einsum("bjrc,bjr->bjc", S["GR"], dAt)
    dR = np.zeros((B, J, 3, 3))
    for j in range(J - 1, 0, -1):
        p = C["parents"][j]
        t = S["Jr"][:, j] - S["Jr"][:, p]
        dR[:, j] = S["GR"][:, p].transpose(0, 2, 1) @ dGR[:, j]
        dt = np.einsum("brc,br->bc", S["GR"][:, p], dGt[:, j])
        dGR[:, p] += dGR[:, j] @ S["R"][:, j].transpose(0, 2, 1) + np.einsum("br,bc->brc", dGt[:, j], t)
        dGt[:, p] += dGt[:, j]
        dJr[:, j] += dt
        dJr[:, p] -= dt
    dR[:, 0] = dGR[:, 0]
    dJr[:, 0] += dGt[:, 0]
    dR[:, 1:] += dc[:, NB:].reshape(B, J - 1, 3, 3)
    d_betas = dc[:, :NB] + np.einsum("jrk,bjr->bk", C["Js"], dJr)
    if np.shape(betas)[0] == 1 and B > 1:
        d_betas = d_betas.sum(0, keepdims=True)
    if pose2rot:
        d_pose = rodrigues_adjoint(S["pose"].reshape(B * J, 3), S["rod"], dR.reshape(B * J, 3, 3)).reshape(np.shape(pose))
    else:
        d_pose = dR.reshape(np.shape(pose))
    return d_betas, d_pose


# ------------------------------------------------------------------------------------------------------------------------- torch restatement
def torch_lbs(betas, pose, P, pose2rot=True):
    """The forward as plain torch ops in the order of smplx/smplx/lbs.py:152-248 (blend_shapes, vertices2joints, batch_rodrigues, pose blend,
    batch_rigid_transform, skinning), in the dtype and on the device of `betas`; P: dict of tensors (parents: a list).  Differentiable."""
    import torch
    B = max(betas.shape[0], pose.shape[0])
    dt, dev = betas.dtype, betas.device
    v_shaped = P["v_template"] + torch.einsum("bl,mkl->bmk", betas, P["shapedirs"])
    Jr = torch.einsum("bik,ji->bjk", v_shaped, P["J_regressor"])
    J = P["J_regressor"].shape[0]
    ident = torch.eye(3, dtype=dt, device=dev)
    if pose2rot:
        rv = pose.reshape(-1, 3)
        angle = torch.norm(rv + 1e-8, dim=1, keepdim=True)
        rot_dir = rv / angle
        cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
        rx, ry, rz = torch.split(rot_dir, 1, dim=1)
        zeros = torch.zeros((rv.shape[0], 1), dtype=dt, device=dev)
        K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(-1, 3, 3)
        rot = (ident[None] + sin * K + (1 - cos) * torch.bmm(K, K)).view(B, J, 3, 3)
    else:
        rot = pose.reshape(B, J, 3, 3)
    pose_feature = (rot[:, 1:] - ident).reshape(B, -1)
    v_posed = torch.matmul(pose_feature, P["posedirs"]).view(B, -1, 3) + v_shaped
    if Jr.shape[0] != B:
        Jr = Jr.expand(B, -1, -1)
    parents = list(P["parents"])
    rel = Jr.clone()
    rel[:, 1:] = Jr[:, 1:] - Jr[:, parents[1:]]
    bottom = torch.tensor([0, 0, 0, 1], dtype=dt, device=dev).view(1, 1, 1, 4).expand(B, J, 1, 4)
    tm = torch.cat([torch.cat([rot, rel.unsqueeze(-1)], dim=3), bottom], dim=2)
    chain = [tm[:, 0]]
    for i in range(1, J):
        chain.append(torch.matmul(chain[parents[i]], tm[:, i]))
    G = torch.stack(chain, dim=1)
    posed = G[:, :, :3, 3]
    jh = torch.cat([Jr, torch.zeros((B, J, 1), dtype=dt, device=dev)], dim=2).unsqueeze(-1)
    A = G - torch.nn.functional.pad(torch.matmul(G, jh), [3, 0, 0, 0, 0, 0, 0, 0])
    T = torch.matmul(P["lbs_weights"].unsqueeze(0).expand(B, -1, -1), A.view(B, J, 16)).view(B, -1, 4, 4)
    vh = torch.cat([v_posed, torch.ones((B, v_posed.shape[1], 1), dtype=dt, device=dev)], dim=2)
    verts = torch.matmul(T, vh.unsqueeze(-1))[:, :, :3, 0]
    return verts, posed


def torch_params(P, dtype, device="cpu"):
    import torch
    out = {k: torch.from_numpy(np.ascontiguousarray(P[k])).to(device=device, dtype=dtype) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")}
    out["parents"] = [int(p) for p in P["parents"]]
    return out


def torch_grads(betas, pose, P, d_verts, d_joints, pose2rot, dtype, device="cpu"):
    """(d_betas, d_pose) of sum(verts * d_verts) + sum(posed * d_joints) by torch autograd of torch_lbs in `dtype`, as float64 numpy arrays."""
    import torch
    tp = torch_params(P, dtype, device)
    b = torch.from_numpy(np.ascontiguousarray(betas)).to(device=device, dtype=dtype).requires_grad_(True)
    p = torch.from_numpy(np.ascontiguousarray(pose)).to(device=device, dtype=dtype).requires_grad_(True)
    verts, posed = torch_lbs(b, p, tp, pose2rot)
    loss = 0
    if d_verts is not None:
        loss = loss + (verts * torch.from_numpy(np.ascontiguousarray(d_verts)).to(device=device, dtype=dtype)).sum()
    if d_joints is not None:
        loss = loss + (posed * torch.from_numpy(np.ascontiguousarray(d_joints)).to(device=device, dtype=dtype)).sum()
    loss.backward()
    return b.grad.double().cpu().numpy(), p.grad.double().cpu().numpy()
