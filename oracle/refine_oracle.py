"""numpy restatement of the garment-skinning / refinement code AROUND the hot path
(modules/mesh_encoder.py:312-487).  TEST INFRASTRUCTURE ONLY.

PINNED (round 5) against the reference's OWN modules/mesh_encoder.py, run in the build container with its absent third-party imports
stubbed (tests/golden/make_golden_refine.py -> tests/golden/refine.npz; tests/test_oracle_golden.py checks lbs_garment_interpolation at
K = 3 and 256, the adjacency of the constructor, and 1 / 3 refinement rounds to 1e-5).  What stays PARITY UNPINNED is `knn_points` alone:
`chamferdist` (krrish94/chamferdist, unpinned in README.md:26) is absent from this image, so the K-nearest search follows the published
behaviour of pytorch3d's knn (squared L2, K smallest, ascending) with tie order = lowest index first -- the same function is the stand-in
inside the golden generator, i.e. the goldens pin everything AROUND the KNN, not the KNN."""
import numpy as np

F32 = np.float32


def knn_points(p1, p2, K=1):
    """(B,P1,3),(B,P2,3) -> dists (B,P1,K) squared L2 ascending, idx (B,P1,K) int64; ties by index."""
    from . import pointnet2_oracle as K_
    d = K_.pairwise_d2(p1.astype(F32), p2.astype(F32))      # `dist += diff*diff` per axis, under the current contraction mode
    idx = np.argsort(d, axis=-1, kind="stable")[..., :K]
    return np.take_along_axis(d, idx, -1), idx.astype(np.int64)


def _interp_weights(d):
    """mesh_encoder.py:341-345 / :375-379: 1/d, inf -> 0, normalise over K, inf -> 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (F32(1.0) / d.astype(F32)).astype(F32)
        w[np.isinf(w)] = 0
        w = (w / w.sum(-1, keepdims=True, dtype=F32)).astype(F32)
        w[np.isinf(w)] = 0
    return w


def lbs_garment_interpolation(garment_t, Tpose_vertices, Tpose_root_joints, zeropose_vertices, parents, gt_pose, T_J_regressor,
                              T_lbs_weights, adj_old, K=3):
    """mesh_encoder.py:312-410 in numpy.  Shapes as in garment4d_amd/garment_lbs.py."""
    import scipy.sparse as sp
    from . import gcn_oracle, lbs_oracle as LO
    B, T = gt_pose.shape[:2]
    J = T_J_regressor.shape[2]
    gt_pose_mat = LO.batch_rodrigues(gt_pose.reshape(-1, 3)).reshape(B * T, 24, 3, 3)
    garment = (garment_t + Tpose_root_joints.reshape(B, 1, 3)).astype(F32)
    body = Tpose_vertices.reshape(B, -1, 3).astype(F32)
    V = body.shape[1]
    dk, ik = knn_points(garment, body, K)
    K64 = min(64, K)
    d64, i64 = dk[..., :K64], ik[..., :K64]
    inv_pose = np.zeros((B, 24, 3), dtype=F32)
    inv_pose[:, 0, 0] = -np.pi / 2; inv_pose[:, 1, 1] = 0.15; inv_pose[:, 2, 1] = -0.15
    inv_pose_mat = LO.batch_rodrigues(inv_pose.reshape(-1, 3)).reshape(B, 24, 3, 3)
    inv_J = LO.vertices2jointsB(T_J_regressor[:, 0], body)
    _, inv_A = LO.batch_rigid_transform(inv_pose_mat, inv_J, parents)
    W0 = T_lbs_weights[:, 0].astype(F32)                                           # (B,V,J)
    w64 = _interp_weights(d64)                                                     # (B,Vg,K64)
    inv_nn_W = np.einsum("bvkj,bvk->bvj", W0[np.arange(B)[:, None, None], i64], w64).astype(F32)   # (nn_W * interp).sum(-2)
    inv_garment = LO.skin(inv_nn_W, inv_A, garment)
    inv_template = np.repeat(inv_garment[:, None], T, 1).reshape(B * T, -1, 3)
    zero_v = zeropose_vertices.reshape(B * T, -1, 3)
    Jf = LO.vertices2jointsB(T_J_regressor.reshape(B * T, J, V), zero_v)
    _, A = LO.batch_rigid_transform(gt_pose_mat, Jf, parents)
    wk = _interp_weights(dk)                                                       # (B,Vg,K)
    Wf = T_lbs_weights.reshape(B, T, V, J).astype(F32)
    nn_W = np.einsum("btvkj,bvk->btvj", Wf[np.arange(B)[:, None, None, None], np.arange(T)[None, :, None, None], ik[:, None]], wk)
    nn_W = nn_W.reshape(B * T, -1, J).astype(F32)
    if K > 1:
        adj = sp.csr_matrix(gcn_oracle.normalize(adj_old) - sp.eye(adj_old.shape[0])).astype(F32)
        Vg = nn_W.shape[1]
        for _ in range(100):
            flat = nn_W.transpose(1, 0, 2).reshape(Vg, -1)
            nn_W = (nn_W + F32(0.1) * adj.dot(flat).astype(F32).reshape(Vg, B * T, J).transpose(1, 0, 2)).astype(F32)
    verts = LO.skin(nn_W, A, inv_template)
    return verts.reshape(B, T, -1, 3), (dk[..., :1], ik[..., :1]), inv_template.reshape(B, T, -1, 3)


# ---------------------------------------------------------------------------------------------------------------------
# The refinement loop of PCALBSGarmentUseSegEncoderSeg.forward (modules/mesh_encoder.py:445-486),
# restated with numpy on top of the pinned pointnet2 / gcn oracles; pinned as a whole by tests/golden/refine.npz (the reference's own
# forward() run with a stub garment encoder: tests/golden/make_golden_refine.py).
def _linear(x, w, b=None):
    y = x.astype(np.float32) @ w.T.astype(np.float32)
    return y if b is None else y + b.astype(np.float32)


def positional_encoding(sd, prefix, radius, nsample, xyz, new_xyz, feats_cm):
    """QueryAndGroup(radius, nsample, use_xyz=True)(xyz, new_xyz, feats (B,C,N)) -> (B,3+C,P,S); permute(0,2,3,1);
    Sequential(Linear, ReLU, Linear); max over the samples (mesh_encoder.py:452-463).  Returns (B,P,Cout)."""
    from . import modules_oracle as MO
    g = MO.query_and_group(radius, nsample, xyz, new_xyz, feats_cm, use_xyz=True)   # (B,3+C,P,S)
    h = np.transpose(g, (0, 2, 3, 1))
    h = np.maximum(_linear(h, sd[prefix + ".0.weight"], sd[prefix + ".0.bias"]), 0)
    h = _linear(h, sd[prefix + ".2.weight"], sd[prefix + ".2.bias"])
    return h.max(axis=-2)


def temporal_attention(last_feat, w_qkv, nbatch, T):
    """mesh_encoder.py:467-476.  last_feat (nbatch*T, Vg, C)."""
    F_, Vg, C = last_feat.shape
    qkv = _linear(last_feat.reshape(nbatch, T, Vg, C), w_qkv)
    q, k, v = [z.reshape(nbatch, T, -1).astype(np.float64) for z in np.split(qkv, 3, axis=-1)]
    a = q @ np.transpose(k, (0, 2, 1)) / np.sqrt(T)
    a = np.exp(a - a.max(-1, keepdims=True))
    a /= a.sum(-1, keepdims=True)
    return (a @ v).reshape(F_, Vg, C).astype(np.float32)


def refinement_head(sd, cur_garment_v, body_v, body_vn, garment_v_list, garment_f_list_pm, adj_csr, nbatch, T,
                    garment_samples=(32, 16, 8), iteration=3, return_ball_idx=False):
    """sd: numpy state dict with the reference's keys.  garment_f_list_pm[i] (F,N_i,C_i) point-major.
    return_ball_idx: also return, per round, the six ball-query index tensors (3 body radii, 3 garment levels) the round's
    positional encoders grouped with -- tests use them to COUNT the queries whose membership differs from the GPU run's."""
    from . import gcn_oracle as GO
    radii = [0.1, 0.2, 0.4]
    body_samples = [8, 16, 32]
    cur = cur_garment_v.astype(np.float32)
    outs, feats = [], []
    body_vn_cm = np.ascontiguousarray(np.transpose(body_vn, (0, 2, 1)))
    gf_cm = [np.ascontiguousarray(np.transpose(f, (0, 2, 1))) for f in garment_f_list_pm]
    ball_idx = []
    for it in range(iteration):
        parts = [cur]
        if return_ball_idx:
            from . import pointnet2_oracle as K_
            ball_idx.append([K_.ball_query(radii[i], body_samples[i], body_v, cur) for i in range(3)]
                            + [K_.ball_query(radii[i], garment_samples[i], garment_v_list[i], cur) for i in range(3)])
        for i in range(3):
            parts.append(positional_encoding(sd, "body_positional_encoding%d" % i, radii[i], body_samples[i], body_v, cur, body_vn_cm))
        for i in range(3):
            parts.append(positional_encoding(sd, "garment_positional_encoding%d" % i, radii[i], garment_samples[i], garment_v_list[i], cur,
                                             gf_cm[i]))
        h = np.concatenate(parts, axis=-1)
        if it > 0:
            h = np.concatenate([h, temporal_attention(feats[-2], sd["temporal_qkv_%d.weight" % it], nbatch, T)], axis=-1)
        for l in range(4):
            p = "lbs_graph_regress%d.%d" % (it + 1, l)
            h = GO.graph_convolution(h, sd[p + ".weight"], sd[p + ".bias"], adj_csr)
            if l != 3:
                h = np.maximum(h, 0)
            feats.append(h)
        cur = cur + h
        outs.append(cur)
    return (outs, ball_idx) if return_ball_idx else outs
