"""Garment skinning by KNN-interpolated body weights -- the immediate caller of the LBS hot path
(`PCALBSGarmentUseSegEncoderSeg.lbs_garment_interpolation`, modules/mesh_encoder.py:312-410).

Same inputs / outputs as the reference method; `body_model.parents` and `self.adj_old` (the un-normalised,
symmetrised garment-mesh adjacency, :299-303) are passed explicitly because this function is not a method of the model.
Differences that do not change results: ONE K-nearest search serves the K, min(64,K) and K=1 queries of :321-324 (the
sorted K=256 list contains the others as prefixes); the (V,J) weight table is never `.repeat`-ed K times -- the blend
kernel gathers rows; the per-frame weights are blended with the clip's neighbour list without materialising the
(B*T, Vg, K, J) tensor of :381-382.  Differentiable in the garment alone: lbs_garment_MGN (the MGN variant's nearest-vertex skinning,
csrc/mgn_skin_grad.hip) always, lbs_garment_interpolation behind tuning.Tuning.garment_lbs_autograd (csrc/skin/skin_grad.hip).
"""
import numpy as np
import torch

from . import _cache
from . import _lib
from . import grad_ops
from . import lbs as L
from . import mesh_tables
from . import tuning
from .gcn import normalize
from .knn import KNN, knn_points


def _blend(W, idx32, dists, frames_per_clip):
    """W (F,V,J), idx32/dists (F/frames_per_clip, Vg, K) -> (F,Vg,J)."""
    F_, V, J = W.shape
    _, Vg, K = idx32.shape
    out = torch.empty((F_, Vg, J), dtype=torch.float32, device=W.device)
    _lib.call("g4d_knn_blend_weights_f32", F_, frames_per_clip, Vg, V, K, J, W.data_ptr(), idx32.data_ptr(), dists.data_ptr(),
              out.data_ptr(), _lib.stream_ptr())
    return out


_operator_cache = {}


def smoothing_operator(adj_old, coeff, iters, device):
    """The `iters` Jacobi steps  W <- W + coeff * ((D^-1 A - I) . W)  are ONE linear map along the vertex axis:
    M = ((1 - coeff) I + coeff D^-1 A)^iters, a dense row-stochastic (Vg,Vg) matrix (100 hops cover the mesh).  Built once
    per mesh by repeated squaring in fp64 on the device, kept in fp32."""
    def build():
        import scipy.sparse as sp
        n = adj_old.shape[0]
        step = (sp.eye(n) * (1.0 - coeff) + normalize(adj_old) * coeff).tocoo()
        base = torch.sparse_coo_tensor(torch.from_numpy(np.vstack((step.row, step.col)).astype(np.int64)), torch.from_numpy(step.data.astype(np.float64)),
                                       (n, n)).to(device).to_dense()
        M, e = None, int(iters)
        while e:                                   # square-and-multiply, fp64 library GEMMs
            if e & 1:
                M = base if M is None else M @ base
            e >>= 1
            if e:
                base = base @ base
        return (torch.eye(n, dtype=torch.float64, device=device) if M is None else M).float().contiguous()

    return _cache.by_identity(_operator_cache, 4, (adj_old,), (float(coeff), int(iters), str(device)), build)


_SMOOTH_OPERATOR_MAX_VG = 8192   # dense operator up to 256 MB; larger meshes run the sparse steps


_smooth_csr_cache = {}


def _smoothing_csr(adj_old, device):
    """(rowptr, colidx, vals, n, longest row) of D^-1 A - I on `device`, built once per adjacency object (scipy work + three H2D
    copies: neither belongs in a forward that may be running under hipGraph capture)."""
    def build():
        import scipy.sparse as sp
        m = mesh_tables.sorted_csr(sp.csr_matrix(normalize(adj_old) - sp.eye(adj_old.shape[0])))
        return mesh_tables.csr_tensors(m, device) + (m.shape[0], mesh_tables.longest_row(m))

    return _cache.by_identity(_smooth_csr_cache, 8, (adj_old,), str(device), build)


_smooth_csr_t_cache = {}


def _smoothing_csr_t(adj_old, device):
    """_smoothing_csr of the TRANSPOSED operator (D^-1 A - I)^T, cached the same way: what the adjoint of the smoothing walks.  A is symmetric in
    its pattern, so the rows have the lengths of the forward operator's and the same kernels serve (row u lists the v with an entry (v, u),
    ascending: mesh_tables.transposed)."""
    def build():
        import scipy.sparse as sp
        m = mesh_tables.transposed(mesh_tables.sorted_csr(sp.csr_matrix(normalize(adj_old) - sp.eye(adj_old.shape[0]))))
        return mesh_tables.csr_tensors(m, device) + (m.shape[0], mesh_tables.longest_row(m))

    return _cache.by_identity(_smooth_csr_t_cache, 8, (adj_old,), str(device), build)


def smooth_weights(nn_W, adj_old, coeff=0.1, iters=100, method=None, transpose=False):
    """100 Jacobi steps  W <- W + coeff * ((D^-1 A - I) . W)  over the garment mesh (:385-390).
    method "jacobi": the steps as written, one SpMM-axpy kernel each (ping-pong buffers).
    method "fused" (default when the mesh fits: mesh_tables.MAX_VG vertices, MAX_ROW entries per adjacency row): all steps in ONE hand-written launch,
    the weights of a (frame, 4-joint slab) resident in LDS (g4d_jacobi_smooth_f32) -- bit-identical to "jacobi".
    method "operator": the same linear map applied as one dense fp32 matrix product (see smoothing_operator; a LIBRARY GEMM,
    kept as a cross-check only); differs from the step-by-step result only by rounding.  G4D_SMOOTH overrides the default.
    transpose=True: the steps of the transposed operator, W <- W + coeff * ((D^-1 A - I)^T . W) -- the adjoint of the smoothing, which is linear
    (the same launches, given _smoothing_csr_t)."""
    import os
    F_, Vg, J = nn_W.shape
    import scipy.sparse as sp
    method = method or os.environ.get("G4D_SMOOTH") or "fused"
    csr = _smoothing_csr_t if transpose else _smoothing_csr
    if method == "fused":
        rowptr, colidx, vals, n, max_row = csr(adj_old, nn_W.device)
        assert n == Vg
        if Vg <= mesh_tables.MAX_VG and max_row <= mesh_tables.MAX_ROW:
            x = nn_W.contiguous()
            out = torch.empty_like(x)
            _lib.call("g4d_jacobi_smooth_f32", F_, Vg, J, int(iters), float(coeff), max_row, x.data_ptr(), rowptr.data_ptr(), colidx.data_ptr(),
                      vals.data_ptr(), out.data_ptr(), _lib.stream_ptr())
            return out
        method = "jacobi"   # mesh too large / too irregular for the LDS-resident kernel: one launch per step
    if method == "operator":
        M = smoothing_operator(adj_old, coeff, iters, nn_W.device)
        M = M.t().contiguous() if transpose else M
        x = nn_W.permute(1, 0, 2).reshape(Vg, F_ * J)                      # vertex-major view of all frames / joints
        return torch.mm(M, x).view(Vg, F_, J).permute(1, 0, 2).contiguous()   # plain library GEMM
    assert method == "jacobi", method
    rowptr, colidx, vals, n, _ = csr(adj_old, nn_W.device)
    assert n == Vg
    a, b, spare = nn_W.contiguous(), torch.empty_like(nn_W), None   # the caller's tensor is read, never written
    st = _lib.stream_ptr()
    for it in range(iters):
        _lib.call("g4d_spmm_axpy_rows_f32", F_, Vg, J, a.data_ptr(), rowptr.data_ptr(), colidx.data_ptr(), vals.data_ptr(), float(coeff),
                  b.data_ptr(), st)
        if it == 0:
            a, b = b, (torch.empty_like(nn_W) if iters > 1 else None)
        else:
            a, b = b, a
    return a


def lbs_garment_interpolation(pred_template_garment_v, Tpose_vertices, Tpose_root_joints, zeropose_vertices, parents, gt_pose,
                              T_J_regressor, T_lbs_weights, adj_old, K=3, clip_J_regressor=None, clip_lbs_weights=None):
    """pred_template_garment_v (B,Vg,3); Tpose_vertices (B,[1,]V,3); Tpose_root_joints (B,[1,]3); zeropose_vertices (B,T,V,3);
    gt_pose (B,T,72); T_J_regressor (B,T,J,V); T_lbs_weights (B,T,V,J); adj_old scipy sparse (Vg,Vg).
    Returns (posed garment (B,T,Vg,3), nearest-neighbour KNN (K=1), un-posed garment repeated over T (B,T,Vg,3)).
    Under tuning.Tuning.garment_lbs_autograd, with grad enabled and a grad-requiring first argument, the posed and the un-posed garment carry a
    graph to that argument (_GarmentSkinFn: the same launches and bits forward, csrc/skin/skin_grad.hip backward); the neighbour lists are
    constants of the graph, as knn_points(...).idx is in the reference, and so are the body, the pose, the regressors and the tables: any of them
    requiring grad raises NotImplementedError.  The nearest-neighbour KNN is never differentiable.  With the flag off nothing here looks at
    requires_grad and no output carries a graph."""
    if tuning.current().garment_lbs_autograd and torch.is_grad_enabled():
        for name, t in (("Tpose_vertices", Tpose_vertices), ("Tpose_root_joints", Tpose_root_joints), ("zeropose_vertices", zeropose_vertices),
                        ("gt_pose", gt_pose), ("T_J_regressor", T_J_regressor), ("T_lbs_weights", T_lbs_weights),
                        ("clip_J_regressor", clip_J_regressor), ("clip_lbs_weights", clip_lbs_weights)):
            if t is not None and t.requires_grad:
                raise NotImplementedError(f"lbs_garment_interpolation: {name} requires grad -- only pred_template_garment_v is differentiated (the "
                                          "body, the pose and the skinning tables are constants of the graph)")
        if pred_template_garment_v.requires_grad:
            B, T = gt_pose.shape[0], gt_pose.shape[1]
            posed, unposed, nn_d, nn_i = _GarmentSkinFn.apply(pred_template_garment_v, Tpose_vertices, Tpose_root_joints, zeropose_vertices, parents,
                                                              gt_pose, T_J_regressor, T_lbs_weights, adj_old, K, clip_J_regressor, clip_lbs_weights)
            stage1 = unposed.reshape(B, 1, -1, 3).repeat(1, T, 1, 1).reshape(B * T, -1, 3).contiguous()
            return posed, KNN(dists=nn_d, idx=nn_i, knn=None), stage1.reshape(B, T, -1, 3)
    return _interpolate(pred_template_garment_v, Tpose_vertices, Tpose_root_joints, zeropose_vertices, parents, gt_pose, T_J_regressor,
                        T_lbs_weights, adj_old, K, clip_J_regressor, clip_lbs_weights)[:3]


def _interpolate(pred_template_garment_v, Tpose_vertices, Tpose_root_joints, zeropose_vertices, parents, gt_pose, T_J_regressor, T_lbs_weights,
                 adj_old, K, clip_J_regressor, clip_lbs_weights):
    """The launches of lbs_garment_interpolation -> its three results and what the adjoint needs of them (see _GarmentSkinFn)."""
    assert pred_template_garment_v.dim() == 3 and pred_template_garment_v.shape[2] == 3
    assert gt_pose.dim() == 3 and gt_pose.shape[2] == 72
    B, T = gt_pose.shape[0], gt_pose.shape[1]
    dev = gt_pose.device
    J = T_J_regressor.shape[2]
    gt_pose_mat = L.batch_rodrigues(gt_pose.reshape(-1, 3).contiguous()).reshape(B * T, 24, 3, 3)
    garment = (pred_template_garment_v + Tpose_root_joints.reshape(B, 3).unsqueeze(1)).contiguous()
    body = Tpose_vertices.reshape(B, -1, 3).contiguous()
    V = body.shape[1]
    nnk = knn_points(garment, body, K=K)                      # :321
    K64 = min(64, K)
    idx_k, d_k = nnk.idx.int().contiguous(), nnk.dists
    idx_64, d_64 = idx_k[..., :K64].contiguous(), d_k[..., :K64].contiguous()   # == knn_points(..., K=K64)  (:323)
    nn1 = KNN(dists=d_k[..., :1].contiguous(), idx=nnk.idx[..., :1].contiguous(), knn=None)  # == knn_points(...)  (:324)

    inv_pose = torch.zeros((B, 24, 3), dtype=torch.float32, device=dev)
    inv_pose[:, 0, 0] = -np.pi / 2
    inv_pose[:, 1, 1] = 0.15
    inv_pose[:, 2, 1] = -0.15
    inv_pose_mat = L.batch_rodrigues(inv_pose.reshape(-1, 3)).reshape(B, 24, 3, 3)
    # the un-posing uses the regressor / weights of the clip's FIRST frame (:333, :338); a rank that holds a later segment of
    # the clip passes them explicitly (clip_J_regressor (B,J,V), clip_lbs_weights (B,V,J))
    cJ = T_J_regressor[:, 0] if clip_J_regressor is None else clip_J_regressor
    cW = T_lbs_weights[:, 0] if clip_lbs_weights is None else clip_lbs_weights
    inv_J = L.vertices2jointsB(cJ.contiguous(), body)
    _, inv_A = L.batch_rigid_transform(inv_pose_mat, inv_J, parents)
    inv_nn_W = _blend(cW.contiguous(), idx_64, d_64, 1)                            # (B,Vg,J)   :339-347
    inv_garment = L.skin(inv_nn_W, inv_A, garment)                                 # :348, :361-362
    inv_template_garment_v = inv_garment.reshape(B, 1, -1, 3).repeat(1, T, 1, 1).reshape(B * T, -1, 3).contiguous()

    zero_v = zeropose_vertices.reshape(B * T, -1, 3).contiguous()
    # A data loader on the GPU (body_models.smpl_clip_batch) hands the per-frame regressor / weights as stride-0 views of
    # ONE table: then the blended, smoothed garment weights are the same for the T frames of a clip and are built once
    # per clip (B rows instead of B*T).  Materialised per-frame copies (the reference's loader) take the general route.
    shared_J = T > 1 and T_J_regressor.stride(1) == 0
    shared_W = T > 1 and T_lbs_weights.stride(1) == 0
    if shared_J:
        Jf = L.vertices2jointsB(T_J_regressor[:, 0].contiguous(), zero_v, group=T)
    else:
        Jf = L.vertices2jointsB(T_J_regressor.reshape(B * T, J, V).contiguous(), zero_v)
    _, A = L.batch_rigid_transform(gt_pose_mat, Jf, parents)
    d_k = d_k.contiguous()
    Wt = T_lbs_weights[:, 0].contiguous() if shared_W else T_lbs_weights.reshape(B * T, V, J).contiguous()
    nn_W = _blend(Wt, idx_k, d_k, 1 if shared_W else T)                            # (B,Vg,J) | (B*T,Vg,J)  :374-382
    if K > 1:
        nn_W = smooth_weights(nn_W, adj_old, 0.1, 100)                             # :385-390
    verts = L.skin(nn_W, A, inv_template_garment_v, group=T if shared_W else 1)   # :393, :406-408
    saved = (garment, body, idx_k, d_k, cW.contiguous(), inv_nn_W, inv_A, inv_garment, Wt, nn_W, A)
    return verts.reshape(B, T, -1, 3), nn1, inv_template_garment_v.reshape(B, T, -1, 3), saved


class _GarmentSkinFn(torch.autograd.Function):
    """lbs_garment_interpolation as an autograd node, differentiable in the T-pose garment alone.  forward = _interpolate (the inference launches,
    same bits) -> (posed (B,T,Vg,3), un-posed (B,Vg,3), and the K = 1 distances / indices, not differentiable).
    Saved: g = x + root, the K neighbour lists and squared distances, both blended weight tensors (the un-posing's and the smoothed posing's),
    inv_A, A, the un-posed garment u; the body and the tables are the caller's (contiguous copies only where the caller's were views).  Nothing
    of the 100 smoothing steps is stored: the smoothing is linear.  At cfg4 (8 clips x 30 frames, Vg 4096, K 256, J 24): lists 2 x 33.6 MB,
    weights 94.4 MB + 3.1 MB per-frame tables / 3.1 MB + 3.1 MB one table per clip, g, u, A, inv_A 1.2 MB: 165.8 MB / 74.6 MB.
    backward (include/g4d_skin.h for the orders): skin adjoint over the clip's frames -> transposed smoothing -> blend adjoint (K) -> skin adjoint of
    the un-posing -> blend adjoint (the min(64, K) prefix): four launches of csrc/skin/skin_grad.hip and one smoothing launch."""

    @staticmethod
    def forward(ctx, x, Tpose_vertices, Tpose_root_joints, zeropose_vertices, parents, gt_pose, T_J_regressor, T_lbs_weights, adj_old, K,
                clip_J_regressor, clip_lbs_weights):
        posed, nn1, _, saved = _interpolate(x, Tpose_vertices, Tpose_root_joints, zeropose_vertices, parents, gt_pose, T_J_regressor, T_lbs_weights,
                                            adj_old, K, clip_J_regressor, clip_lbs_weights)
        ctx.adj_old, ctx.K, ctx.T = adj_old, int(K), int(gt_pose.shape[1])
        ctx.save_for_backward(*saved)
        ctx.mark_non_differentiable(nn1.dists, nn1.idx)
        return posed, saved[7], nn1.dists, nn1.idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_posed, d_unposed, _d_dists, _d_idx):
        g, body, idx_k, d_k, cW, inv_nn_W, inv_A, u, Wt, nn_W, A = ctx.saved_tensors
        B, Vg, K, T = g.shape[0], g.shape[1], ctx.K, ctx.T
        shared = Wt.shape[0] == B and T > 1
        du = None if d_unposed is None else d_unposed.float().contiguous()
        dg = None
        if d_posed is not None:
            dy = d_posed.float().reshape(B * T, Vg, 3).contiguous()
            du, d_nn_W = grad_ops.garment_skin_grad(B, T, nn_W, A, u, dy, d_add=du)
            if K > 1:
                d_nn_W = smooth_weights(d_nn_W, ctx.adj_old, 0.1, 100, transpose=True)
            dg = grad_ops.knn_blend_grad(Wt, 1 if shared else T, idx_k, d_k, K, d_nn_W, g, body)
        if du is None:
            return (torch.zeros_like(g),) + (None,) * 11
        dg, d_inv_W = grad_ops.garment_skin_grad(B, 1, inv_nn_W, inv_A, g, du, d_add=dg)
        dg = grad_ops.knn_blend_grad(cW, 1, idx_k, d_k, min(64, K), d_inv_W, g, body, d_add=dg)
        return (dg,) + (None,) * 11


def _inv_template_pose_mats(F_, device):
    """The fixed inverse template pose of :543-546 (root -pi/2 about x, hips +-0.15 about y) as (F,24,3,3) rotation matrices."""
    inv_pose = torch.zeros((1, 24, 3), dtype=torch.float32, device=device)
    inv_pose[:, 0, 0] = -np.pi / 2
    inv_pose[:, 1, 1] = 0.15
    inv_pose[:, 2, 1] = -0.15
    return L.batch_rodrigues(inv_pose.reshape(-1, 3)).reshape(1, 24, 3, 3).expand(F_, 24, 3, 3).contiguous()


class _MGNSkinFn(torch.autograd.Function):
    """g4d_mgn_skin_f32 as an autograd node, differentiable in the garment alone.  forward = the inference launch (same bits); saved: the nearest
    index and the three tables both blends read; backward = ONE launch of g4d_mgn_skin_grad_f32 (csrc/mgn_skin_grad.hip), which recomputes the
    blends at the saved index.  Outputs: (posed, stage 1, index, squared distance); index and distance are not differentiable."""

    @staticmethod
    def forward(ctx, garment, root, body, W, inv_A, A, clips, T):
        idx, dists, stage1, posed = _mgn_skin(clips, T, garment, root, body, W, inv_A, A)
        ctx.clips, ctx.T = clips, T
        ctx.save_for_backward(idx, W, inv_A, A)
        ctx.mark_non_differentiable(idx, dists)
        return posed, stage1, idx, dists

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_posed, d_stage1, _d_idx, _d_dists):
        idx, W, inv_A, A = ctx.saved_tensors
        if d_posed is None:                        # only stage 1 was used downstream
            d_posed = torch.zeros((idx.shape[0], idx.shape[1], 3), dtype=torch.float32, device=idx.device)
        d_posed = d_posed.float().contiguous()
        if d_stage1 is not None:
            d_stage1 = d_stage1.float().contiguous()
        return (grad_ops.mgn_skin_grad(ctx.clips, ctx.T, idx, W, inv_A, A, d_posed, d_stage1),) + (None,) * 7


def _mgn_skin(clips, T, garment, root, body, W, inv_A, A):
    """The one call site of g4d_mgn_skin_f32 -> (idx (F,Vg,1) int32, dists (F,Vg,1), stage1 (F,Vg,3), posed (F,Vg,3))."""
    F_, Vg = garment.shape[0], garment.shape[1]
    V, J = body.shape[1], W.shape[2]
    dev = garment.device
    idx = torch.empty((F_, Vg, 1), dtype=torch.int32, device=dev)
    dists = torch.empty((F_, Vg, 1), dtype=torch.float32, device=dev)
    stage1 = torch.empty((F_, Vg, 3), dtype=torch.float32, device=dev)
    posed = torch.empty((F_, Vg, 3), dtype=torch.float32, device=dev)
    _lib.call("g4d_mgn_skin_f32", clips, T, Vg, V, J, garment.data_ptr(), root.data_ptr(), body.data_ptr(), W.data_ptr(), inv_A.data_ptr(),
              A.data_ptr(), idx.data_ptr(), dists.data_ptr(), stage1.data_ptr(), posed.data_ptr(), _lib.stream_ptr())
    return idx, dists, stage1, posed


def lbs_garment_MGN(pred_template_garment_v, Tpose_vertices, Tpose_root_joints, zeropose_vertices, parents, gt_pose, T_J_regressor,
                    T_lbs_weights, K=1):
    """`PCALBSGarmentUseSegEncoderSegMGN.lbs_garment_MGN` (modules/mesh_encoder.py:529-585).  pred_template_garment_v (B,T,Vg,3);
    Tpose_vertices (B,[1,]V,3); Tpose_root_joints (B,[1,]3); zeropose_vertices (B,T,V,3); gt_pose (B,T,72); T_J_regressor (B,T,J,V);
    T_lbs_weights (B,T,V,J).  Returns (posed (B,T,Vg,3), nearest body vertex KNN with dists / idx (B*T,Vg,1), stage 1 = the garment
    un-posed by the inverse template pose (B,T,Vg,3)).
    The joints and the two sets of joint transforms come from the lbs helpers (inv_A: per-frame regressor on the clip's T-pose, :548-550;
    A: per-frame regressor on the zero-pose vertices, :562-564); the K = 1 search and both blends at the nearest vertex are ONE launch
    (g4d_mgn_skin_f32): the (B*T, V, 4, 4) blends of :553 / :568 never exist.
    Differentiable in its FIRST argument (posed and stage 1; the nearest index is a constant of the graph, as knn_points(...).idx is in the
    reference): under grad with a grad-requiring garment the same launch runs as an autograd node whose backward is g4d_mgn_skin_grad_f32.
    Any other input that requires grad raises NotImplementedError; the nearest-vertex KNN is never differentiable."""
    assert pred_template_garment_v.dim() == 4 and pred_template_garment_v.shape[-1] == 3
    assert gt_pose.dim() == 3 and gt_pose.shape[2] == 72
    assert K == 1
    train = torch.is_grad_enabled() and pred_template_garment_v.requires_grad
    if torch.is_grad_enabled():
        for name, t in (("Tpose_vertices", Tpose_vertices), ("Tpose_root_joints", Tpose_root_joints), ("zeropose_vertices", zeropose_vertices),
                        ("gt_pose", gt_pose), ("T_J_regressor", T_J_regressor), ("T_lbs_weights", T_lbs_weights)):
            if t.requires_grad:
                raise NotImplementedError(f"lbs_garment_MGN: {name} requires grad -- only pred_template_garment_v is differentiated (the body, the "
                                          "pose and the skinning tables are constants of the graph)")
    B, T = gt_pose.shape[0], gt_pose.shape[1]
    F_ = B * T
    dev = gt_pose.device
    Vg = pred_template_garment_v.shape[2]
    J = T_J_regressor.shape[2]
    garment = L._f32(pred_template_garment_v, "pred_template_garment_v").reshape(F_, Vg, 3)
    with torch.no_grad():
        body = L._f32(Tpose_vertices, "Tpose_vertices").reshape(B, -1, 3)
        V = body.shape[1]
        root = L._f32(Tpose_root_joints, "Tpose_root_joints").reshape(B, 3)
        Jreg = L._f32(T_J_regressor, "T_J_regressor").reshape(F_, J, V)
        W = L._f32(T_lbs_weights, "T_lbs_weights").reshape(F_, V, J)
        if not (tuple(pred_template_garment_v.shape[:2]) == (B, T) and tuple(T_lbs_weights.shape) == (B, T, V, J)
                and tuple(T_J_regressor.shape) == (B, T, J, V) and zeropose_vertices.numel() == F_ * V * 3):
            raise RuntimeError("lbs_garment_MGN: inputs disagree on (B, T, Vg, V, J)")
        gt_pose_mat = L.batch_rodrigues(gt_pose.reshape(-1, 3).contiguous()).reshape(F_, 24, 3, 3)
        body_f = body.reshape(B, 1, V, 3).expand(B, T, V, 3).reshape(F_, V, 3)       # new_Tpose_vertices (:540)
        _, inv_A = L.batch_rigid_transform(_inv_template_pose_mats(F_, dev), L.vertices2jointsB(Jreg, body_f), parents)
        Jz = L.vertices2jointsB(Jreg, zeropose_vertices.reshape(F_, V, 3))
        _, A = L.batch_rigid_transform(gt_pose_mat, Jz, parents)
    if train:
        posed, stage1, idx, dists = _MGNSkinFn.apply(garment, root, body, W, inv_A, A, B, T)
    else:
        with torch.no_grad():
            idx, dists, stage1, posed = _mgn_skin(B, T, garment, root, body, W, inv_A, A)
    return posed.reshape(B, T, Vg, 3), KNN(dists=dists, idx=idx.long(), knn=None), stage1.reshape(B, T, Vg, 3)
