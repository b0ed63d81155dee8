"""Losses that share the kernels of the hot path.
`calc_interpenetration_loss` (smplx/loss/temporal_loss.py:20-46), forward only = vertex normals + nearest body vertex +
penalty, each on a HIP kernel.  The nearest vertex comes from the three-nearest-neighbour kernel of the feature-propagation
layers (ties -> lowest index, like knn_points here), not from a K=1 top-K search.
`temporal_loss_PCA_LBS` (:147-201), the stage-2 objective of the refinement head, with its analytic gradient w.r.t. the round outputs
(csrc/refine_loss.hip); `stage2_loss` is the same on plain tensors.
`temporal_loss_PCA` (:60-119), the stage-1 objective of the garment encoder, with its analytic gradient w.r.t. the logits, the PCA coefficients
and the T-pose garment (csrc/stage1_loss.hip); `stage1_loss` is the same on plain tensors."""
import numpy as np
import torch

from . import _cache
from . import _lib
from . import fused
from . import mesh_tables
from . import mesh_utils

_vf = {}


def interpenetration_per_vertex(body_v, body_vn, garment_v):
    """body_v / body_vn (F,V,3), garment_v (F,Vg,3) -> (penalty (F,Vg), nearest body vertex (F,Vg) int64)."""
    F_, V, _ = body_v.shape
    Vg = garment_v.shape[1]
    dev = body_v.device
    st = _lib.stream_ptr()
    g, b, n = garment_v.contiguous(), body_v.contiguous(), body_vn.contiguous()
    _, idx = fused.three_nn(g, b)
    pen = torch.empty((F_, Vg), dtype=torch.float32, device=dev)
    _lib.call("g4d_interpenetration_f32", F_, Vg, V, g.data_ptr(), b.data_ptr(), n.data_ptr(), idx.data_ptr(), 3, pen.data_ptr(), st)
    return pen, idx[..., 0].long()


@torch.no_grad()
def calc_interpenetration_loss(body_model, so, garment_v, reduce_fn="sum", to_root_joint=False):
    """Same arguments as the reference: so['vertices'] (F,V,3), so['joints'] (F,>=1,3); garment_v (F,Vg,3) or (B,T,Vg,3)."""
    assert body_model.faces.shape[1] == 3 and so["vertices"].shape[1] >= 3, "body needs triangle faces and >= 3 vertices"
    key = id(body_model)
    if key not in _vf:
        fid, vid = mesh_utils.calc_body_mesh_info(body_model)
        _vf.clear()
        _vf[key] = (fid.cuda(), vid.cuda(), torch.from_numpy(np.asarray(body_model.faces).astype(np.int64)).cuda())
    fid, vid, faces = _vf[key]
    if garment_v.dim() == 4:
        garment_v = garment_v.reshape(garment_v.shape[0] * garment_v.shape[1], garment_v.shape[2], 3)
    verts = so["vertices"].float()
    vn = mesh_utils.compute_vnorms(verts, faces, vid, fid)
    g = garment_v + so["joints"][:, 0, :].unsqueeze(1) if to_root_joint else garment_v
    pen, _ = interpenetration_per_vertex(verts, vn, g.float())
    if reduce_fn == "sum":
        return pen.sum(-1).mean()
    if reduce_fn == "mean":
        return pen.mean()
    raise NotImplementedError


# ------------------------------------------------------------------------------------------------------------ the stage-2 objective
# `temporal_loss_PCA_LBS` (smplx/loss/temporal_loss.py:147-201): the function whose total_loss.backward() trains the refinement head in the
# reference's second stage (train_temporal.py --fix_PCA).  Values and dL/d(round output) come from csrc/refine_loss.hip, one call per round;
# what is in front of the rounds (targets, body, normals, the nearest-vertex index) is constant, as in the reference.
LOSS_LAMBDAS = ("LBS_GARMENT_L2_LOSS_LAMBDA", "LBS_GARMENT_LAP_LOSS_LAMBDA", "LBS_INTERPENETRATION_LOSS_LAMBDA", "TEMPORAL_CONSTRAINT_LOSS_LAMBDA")
_lap_cache = {}


def laplacian_csr(lap_adj, device):
    """The operands of g4d_refine_loss_f32 for the mesh Laplacian `lap_adj` (the model's output_dict['lap_adj'], a torch sparse (Vg, Vg)
    tensor, or a scipy sparse matrix): (rowptr, colidx, vals, rowsum, rowptr_t, colidx_t, vals_t), i.e. the CSR of L, its row sums (float64
    sums of the fp32 entries) and the CSR of L^T (L's pattern on a symmetric mesh, values -1/deg of the OTHER vertex), all on `device`.
    Recovered from the matrix itself -- whatever the caller built it from -- once per object (cached by identity, like
    garment_lbs._smoothing_csr): scipy work and seven host-to-device copies, which do not belong inside a hipGraph capture."""
    def build():
        assert not torch.cuda.is_current_stream_capturing(), "laplacian_csr: build the operator before the capture (call the loss once eagerly)"
        L = mesh_tables.sorted_csr(lap_adj).astype(np.float32)
        assert L.shape[0] == L.shape[1], "the Laplacian is square"
        L.sum_duplicates()
        rowsum = np.asarray(L.astype(np.float64).sum(1)).reshape(-1)
        return (mesh_tables.csr_tensors(L, device) + (mesh_tables.to_device(rowsum, np.float32, device),)
                + mesh_tables.csr_tensors(mesh_tables.transposed(L), device))

    return _cache.by_identity(_lap_cache, 8, (lap_adj,), str(device), build)


def _lambdas(loss_cfg):
    get = (lambda k: loss_cfg[k]) if isinstance(loss_cfg, dict) else (lambda k: getattr(loss_cfg, k))
    return tuple(float(get(k)) for k in LOSS_LAMBDAS)


def _evaluate_rounds(rounds, want, target, body_v, body_vn, csr, nbatch, T, weights):
    """One g4d_refine_loss_f32 call per round.  Returns (vals (R, 5) = [L2, MSRE, Laplacian, penetration, temporal] per round -- the temporal
    term evaluated for the last round only --, msre_frames (F) of the last round, [dL/d round or None])."""
    R = len(rounds)
    F_, Vg, _ = rounds[0].shape
    V = body_v.shape[1]
    dev = body_v.device
    vals = torch.empty((R, 5), dtype=torch.float32, device=dev)
    msre = torch.empty((F_,), dtype=torch.float32, device=dev)
    ws = _lib.workspace(_lib.lib().g4d_refine_loss_ws_bytes(F_, Vg, int(any(want))), dev)   # one workspace: the rounds run in stream order
    grads = []
    st = _lib.stream_ptr()
    for r, p in enumerate(rounds):
        p = p.detach().float().contiguous()
        assert p.shape == (F_, Vg, 3), "every round's prediction is (nbatch * T, Vg, 3)"
        idx = fused.three_nn(p, body_v)[1] if F_ * Vg else torch.zeros((F_, Vg, 3), dtype=torch.int32, device=dev)
        g = torch.empty_like(p) if want[r] else None
        last = r == R - 1
        _lib.call("g4d_refine_loss_f32", nbatch, T, Vg, V, p.data_ptr(), target.data_ptr(), body_v.data_ptr(), body_vn.data_ptr(), idx.data_ptr(), 3,
                  *[t.data_ptr() for t in csr], weights[0], weights[1], weights[2], weights[3] if last else 0.0, int(last), ws.data_ptr(),
                  vals[r].data_ptr(), msre.data_ptr() if last else 0, 0 if g is None else g.data_ptr(), st)
        grads.append(g)
    return vals, msre, grads


def _total(vals, weights):
    acc = vals.sum(0)
    return (acc[0] * weights[0] + acc[2] * weights[1] + acc[3] * weights[2]) + vals[-1, 4] * weights[3]


class _Stage2LossFn(torch.autograd.Function):
    """total_loss over the round outputs: the forward evaluates every round and keeps dL/d(round) of those that require grad; the backward
    hands each its stored gradient times the incoming scalar."""

    @staticmethod
    def forward(ctx, consts, *rounds):
        target, body_v, body_vn, csr, nbatch, T, weights = consts
        want = [bool(n) for n in ctx.needs_input_grad[1:]]
        vals, msre, grads = _evaluate_rounds(rounds, want, target, body_v, body_vn, csr, nbatch, T, weights)
        ctx.want = want
        ctx.save_for_backward(*[g for g in grads if g is not None])
        ctx.mark_non_differentiable(vals, msre)
        return _total(vals, weights), vals, msre

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total, _g_vals, _g_msre):
        saved = iter(ctx.saved_tensors)
        return (None,) + tuple((next(saved) * g_total) if w else None for w in ctx.want)


def stage2_loss(rounds, target, body_v, body_vn, lap_adj, nbatch, T, weights):
    """The objective on tensors: rounds = the per-round predictions (F, Vg, 3), F = nbatch * T; target (F, Vg, 3); body_v / body_vn (F, V, 3)
    body vertices / unit normals; lap_adj the mesh Laplacian (see laplacian_csr); weights = the four lambdas (L2, Laplacian, penetration,
    temporal).  Returns (total, vals (R, 5), msre_frames (F,)); `total` carries the graph when grad is enabled and a round requires grad,
    `vals` / `msre_frames` never do.  Without grad: the same launches without gradient buffers, the same bits."""
    rounds = list(rounds)
    assert len(rounds) >= 1 and all(p.dim() == 3 and p.shape[-1] == 3 for p in rounds)
    if torch.is_grad_enabled():
        for name, t in (("target", target), ("body_v", body_v), ("body_vn", body_vn)):
            if t.requires_grad:
                raise NotImplementedError(f"stage-2 loss: {name} requires grad -- only the round outputs are differentiated (targets, body vertices and "
                                          "normals are constants of the graph, as in the reference's second stage)")
    dev = rounds[0].device
    with torch.no_grad():
        target, body_v, body_vn = (t.detach().to(dev).float().contiguous() for t in (target, body_v, body_vn))
    F_, Vg, _ = rounds[0].shape
    assert F_ == nbatch * T and target.shape == (F_, Vg, 3) and body_v.shape == body_vn.shape and body_v.shape[0] == F_
    csr = laplacian_csr(lap_adj, dev)
    assert csr[0].numel() == Vg + 1, "lap_adj is (Vg, Vg)"
    weights = tuple(float(w) for w in weights)
    if torch.is_grad_enabled() and any(p.requires_grad for p in rounds):
        return _Stage2LossFn.apply((target, body_v, body_vn, csr, nbatch, T, weights), *rounds)
    with torch.no_grad():
        vals, msre, _ = _evaluate_rounds(rounds, [False] * len(rounds), target, body_v, body_vn, csr, nbatch, T, weights)
        return _total(vals, weights), vals, msre


def _acceleration_error(pred, gt, nbatch, T):
    """calc_acceleration_error (:133-145); an evaluation figure outside total_loss."""
    def accel(v):
        v = v.reshape(nbatch, T, -1, 3)
        vel = (v[:, 1:] - v[:, :-1]) / (1 / 30)
        return (vel[:, 1:] - vel[:, :-1]) / (1 / 30)
    return ((accel(pred) - accel(gt)) ** 2).sum(-1).sqrt().mean()


def temporal_loss_PCA_LBS(output_dict, inputs, body_model, args=None, *, loss_cfg):
    """The reference's four positional arguments (`args` is not read) plus loss_cfg: anything with the four LBS_* / TEMPORAL_* lambdas as
    attributes (cfg.LOSS) or a dict.  Reads output_dict['iter_regressed_lbs_garment_v' | 'lbs_pred_garment_v' | 'lap_adj'] and
    inputs['pose_torch' | 'smpl_vertices_torch' | 'smpl_root_joints_torch' | 'garment_torch']; returns the reference's loss_dict keys.
    `total_loss` is differentiable w.r.t. the round outputs (one autograd node on csrc/refine_loss.hip); every other entry is a detached
    figure.  The Laplacian's CSR is recovered from `lap_adj` itself, once per object (laplacian_csr)."""
    weights = _lambdas(loss_cfg)
    rounds = list(output_dict["iter_regressed_lbs_garment_v"])
    dev = rounds[0].device
    nbatch, T = inputs["pose_torch"].shape[0], inputs["pose_torch"].shape[1]
    F_ = nbatch * T
    if torch.is_grad_enabled():
        for k in ("garment_torch", "smpl_vertices_torch", "smpl_root_joints_torch"):
            if inputs[k].requires_grad:
                raise NotImplementedError(f"temporal_loss_PCA_LBS: inputs['{k}'] requires grad -- only the round outputs are differentiated")
    with torch.no_grad():
        body_v = inputs["smpl_vertices_torch"].to(dev).reshape(F_, -1, 3).float().contiguous()
        joints = inputs["smpl_root_joints_torch"].to(dev).reshape(F_, 1, 3).float()
        gt = (inputs["garment_torch"].to(dev).reshape(F_, -1, 3).float() + joints[:, 0, :].unsqueeze(1)).contiguous()
        assert body_model.faces.shape[1] == 3 and body_v.shape[1] >= 3, "body needs triangle faces and >= 3 vertices"
        key = id(body_model)
        if key not in _vf:
            fid, vid = mesh_utils.calc_body_mesh_info(body_model)
            _vf.clear()
            _vf[key] = (fid.cuda(), vid.cuda(), torch.from_numpy(np.asarray(body_model.faces).astype(np.int64)).cuda())
        fid, vid, faces = _vf[key]
        body_vn = mesh_utils.compute_vnorms(body_v, faces, vid, fid)
    rounds = [p.reshape(F_, -1, 3) for p in rounds]
    total, vals, msre = stage2_loss(rounds, gt, body_v, body_vn, output_dict["lap_adj"], nbatch, T, weights)
    with torch.no_grad():
        acc = vals.sum(0)
        lbs_pred = output_dict["lbs_pred_garment_v"].detach().to(dev).reshape(F_, -1, 3).float()
        last = rounds[-1].detach()
        return {
            "lbs_garment_msre": vals[-1, 1], "lbs_garment_msre_list": msre.reshape(nbatch, T),
            "only_lbs_garment_msre": ((lbs_pred - gt) ** 2).sum(-1).sqrt().mean(),
            "lbs_garment_l2_loss": acc[0], "lbs_garment_lap_loss": acc[2], "lbs_interpenetration_loss": acc[3],
            "temporal_constraint_loss": vals[-1, 4],
            "acceleration_error": _acceleration_error(last, gt, nbatch, T),
            "only_lbs_acceleration_error": _acceleration_error(lbs_pred, gt, nbatch, T),
            "total_loss": total,
        }


# ------------------------------------------------------------------------------------------------------------ the stage-1 objective
# `temporal_loss_PCA` (smplx/loss/temporal_loss.py:60-119): the function whose total_loss.backward() trains the garment encoder in the
# reference's first stage.  Values and the analytic gradient w.r.t. the logits, the PCA coefficients and the T-pose garment come from
# csrc/stage1_loss.hip; targets, the T-pose body, its normals and the nearest-vertex index are constants, as in the reference -- and so is the
# cotangent Laplacian, which the reference rebuilds from the predicted vertices on every call and holds fixed in its backward.
STAGE1_LAMBDAS = ("SEM_SEG_LOSS_LAMBDA", "GARMENT_PCA_COEFF_L2_LAMBDA", "GARMENT_L2_LOSS_LAMBDA", "INTERPENETRATION_LOSS_LAMBDA", "GARMENT_LAP_LOSS_LAMBDA")
STAGE1_VALUES = ("sem_seg_loss", "garment_pca_coeff_l2", "garment_l2_loss", "garment_msre", "interpenetration_loss", "garment_lap_loss")
_inc_cache = {}


def face_incidence(faces3, vg, device):
    """The operands of g4d_stage1_garment_f32 for the triangle array `faces3` (nf, 3) (the model's output_dict['garment_f_3']): (faces int32
    (nf, 3), inc_rowptr (vg + 1), inc) on `device`, inc holding face * 3 + corner for every corner of vertex i between inc_rowptr[i] and
    inc_rowptr[i + 1], in face order.  Built on the host once per array (cached by identity, like laplacian_csr): not inside a hipGraph capture."""
    def build():
        assert torch.device(device).type != "cuda" or not torch.cuda.is_current_stream_capturing(), "face_incidence: build the incidence before the capture (call the loss once eagerly)"
        f = faces3.detach().cpu().numpy() if torch.is_tensor(faces3) else np.asarray(faces3)
        f = np.ascontiguousarray(f.reshape(-1, 3).astype(np.int64))
        assert f.size == 0 or (f.min() >= 0 and f.max() < vg), "a face names a vertex outside the garment"
        rowptr, corners = mesh_tables.vertex_corners(f, vg)        # entry = face * 3 + corner, ascending within a vertex
        return tuple(mesh_tables.to_device(a, np.int32, device) for a in (f, rowptr, corners))

    return _cache.by_identity(_inc_cache, 8, (faces3,), (int(vg), str(device)), build)


def _stage1_lambdas(loss_cfg):
    get = (lambda k: loss_cfg[k]) if isinstance(loss_cfg, dict) else (lambda k: getattr(loss_cfg, k))
    return tuple(float(get(k)) for k in STAGE1_LAMBDAS)


def _evaluate_stage1(logits, coeff, pred, want, consts):
    """The launches of csrc/stage1_loss.hip.  Returns (vals (6,) in STAGE1_VALUES order, [d total / d logits, d coeff, d pred] or None each)."""
    labels, coeff_gt, target, root, body_v, body_vn, inc, pad_batch, weights, only_seg = consts
    dev = logits.device
    st = _lib.stream_ptr()
    L = _lib.lib()
    vals = torch.zeros(6, dtype=torch.float32, device=dev)
    x = logits.detach().float().contiguous()
    C = x.shape[-1]
    rows = x.numel() // C if C else 0
    assert labels.numel() == rows, "one label per row of logits"
    g_logits = torch.empty_like(x) if want[0] else None
    ws = _lib.workspace(L.g4d_stage1_loss_ws_bytes(rows, 0, 0, 0, 0), dev)
    _lib.call("g4d_stage1_ce_f32", rows, C, x.data_ptr(), labels.data_ptr(), weights[0], ws.data_ptr(), vals.data_ptr(),
              0 if g_logits is None else g_logits.data_ptr(), st)
    if only_seg:
        return vals, [g_logits, None, None]
    a, p = coeff.detach().float().contiguous(), pred.detach().float().contiguous()
    B, Vg, _ = p.shape
    V, P = body_v.shape[1], a.shape[1]
    faces, rowptr, entries = inc
    nf = faces.shape[0]
    q = p + root[:, None, :]
    idx = fused.three_nn(q, body_v)[1] if B * Vg else torch.zeros((B, Vg, 3), dtype=torch.int32, device=dev)
    g_coeff = torch.empty_like(a) if want[1] else None
    g_pred = torch.empty_like(p) if want[2] else None
    ws = _lib.workspace(L.g4d_stage1_loss_ws_bytes(0, B, Vg, nf, int(want[2])), dev)
    out = torch.empty(5, dtype=torch.float32, device=dev)
    _lib.call("g4d_stage1_garment_f32", B, pad_batch, Vg, V, nf, P, p.data_ptr(), target.data_ptr(), root.data_ptr(), body_v.data_ptr(), body_vn.data_ptr(),
              idx.data_ptr(), 3, faces.data_ptr(), rowptr.data_ptr(), entries.data_ptr(), a.data_ptr(), coeff_gt.data_ptr(), weights[1], weights[2],
              weights[3], weights[4], ws.data_ptr(), out.data_ptr(), 0 if g_pred is None else g_pred.data_ptr(),
              0 if g_coeff is None else g_coeff.data_ptr(), st)
    vals[1], vals[2:6] = out[4], out[0:4]
    return vals, [g_logits, g_coeff, g_pred]


def _stage1_total(vals, weights, only_seg):
    """The reference's accumulation order (the MSRE, vals[3], is reported but not part of the total)."""
    total = vals[0] * weights[0]
    if only_seg:
        return total
    return (((total + vals[1] * weights[1]) + vals[2] * weights[2]) + vals[4] * weights[3]) + vals[5] * weights[4]


class _Stage1LossFn(torch.autograd.Function):
    """total_loss over (logits, coefficients, T-pose garment): the forward evaluates the objective and keeps the gradients of the inputs that
    require grad; the backward hands each its stored gradient times the incoming scalar."""

    @staticmethod
    def forward(ctx, consts, logits, coeff, pred):
        want = [bool(n) for n in ctx.needs_input_grad[1:]]
        vals, grads = _evaluate_stage1(logits, coeff, pred, want, consts)
        ctx.want = [w and g is not None for w, g in zip(want, grads)]
        ctx.shapes = [None if t is None else t.shape for t in (logits, coeff, pred)]
        ctx.save_for_backward(*[g for g, w in zip(grads, ctx.want) if w])
        ctx.mark_non_differentiable(vals)
        return _stage1_total(vals, consts[8], consts[9]), vals

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total, _g_vals):
        saved = iter(ctx.saved_tensors)
        return (None,) + tuple((next(saved) * g_total).reshape(s) if w else None for w, s in zip(ctx.want, ctx.shapes))


def stage1_loss(sem_logits, labels, coeff, coeff_gt, tpose_garment, garment_gt, root, body_v, body_vn, faces3, pad_batch, weights, only_seg=False):
    """The objective on tensors: sem_logits (..., C) point-major with one int label per row; coeff / coeff_gt (B, P); tpose_garment / garment_gt
    (B, Vg, 3); root (B, 3) the T-pose root joints; body_v / body_vn (B, V, 3) the T-pose body and its unit normals; faces3 (nf, 3) the garment's
    triangles (see face_incidence); pad_batch >= B the batch size the Laplacian term is padded to with copies of item 0; weights = the five
    lambdas in STAGE1_LAMBDAS order.  With only_seg only sem_logits and labels are read.  Returns (total, vals (6,) in STAGE1_VALUES order,
    zeros behind the first under only_seg); `total` carries the graph when grad is enabled and one of sem_logits, coeff, tpose_garment requires
    grad, `vals` never does.  Without grad: the same launches without gradient buffers, the same bits."""
    weights = tuple(float(w) for w in weights)
    assert len(weights) == 5
    consts_in = (("labels", labels),) if only_seg else (("labels", labels), ("coeff_gt", coeff_gt), ("garment_gt", garment_gt), ("root", root),
                                                        ("body_v", body_v), ("body_vn", body_vn))
    if torch.is_grad_enabled():
        for name, t in consts_in:
            if t.requires_grad:
                raise NotImplementedError(f"stage-1 loss: {name} requires grad -- only the logits, the PCA coefficients and the T-pose garment are "
                                          "differentiated (targets, body vertices and normals are constants of the graph, as in the reference's first stage)")
    dev = sem_logits.device
    with torch.no_grad():
        labels = labels.detach().to(dev).reshape(-1).long().contiguous()
        if only_seg:
            consts = (labels, None, None, None, None, None, None, 0, weights, True)
            coeff = tpose_garment = None
        else:
            coeff_gt, garment_gt, root, body_v, body_vn = (t.detach().to(dev).float().contiguous() for t in (coeff_gt, garment_gt, root, body_v, body_vn))
            B, Vg, _ = tpose_garment.shape
            assert garment_gt.shape == (B, Vg, 3) and root.shape == (B, 3) and body_v.shape == body_vn.shape and body_v.shape[0] == B
            assert coeff.shape == coeff_gt.shape and coeff.shape[0] == B and int(pad_batch) >= B, "pad_batch (args.batch_size) is at least the batch"
            consts = (labels, coeff_gt, garment_gt, root, body_v, body_vn, face_incidence(faces3, Vg, dev), int(pad_batch), weights, False)
    leaves = [t for t in (sem_logits, coeff, tpose_garment) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in leaves):
        return _Stage1LossFn.apply(consts, sem_logits, coeff, tpose_garment)
    with torch.no_grad():
        vals, _ = _evaluate_stage1(sem_logits, coeff, tpose_garment, [False] * 3, consts)
        return _stage1_total(vals, weights, only_seg), vals


def temporal_loss_PCA(output_dict, inputs, body_model, args, *, loss_cfg):
    """The reference's four positional arguments (`args.only_seg` and `args.batch_size` are read) plus loss_cfg: anything with the five lambdas
    of STAGE1_LAMBDAS as attributes (cfg.LOSS) or a dict.  Reads output_dict['sem_logits' | 'garment_PCA_coeff' | 'tpose_garment' | 'garment_f_3']
    and inputs['pose_torch' | 'pcd_label_torch' | 'PCACoeff' | 'garment_template_vertices' | 'Tpose_smpl_vertices_torch' |
    'Tpose_smpl_root_joints_torch']; returns the reference's loss_dict keys (the first and the last only with args.only_seg).  The numbers of
    points, classes and PCA coefficients come from the tensors' shapes.  `total_loss` is differentiable w.r.t. the logits, the coefficients and
    the T-pose garment (one autograd node on csrc/stage1_loss.hip); every other entry is a detached figure."""
    weights = _stage1_lambdas(loss_cfg)
    logits = output_dict["sem_logits"]
    dev = logits.device
    B = inputs["pose_torch"].shape[0]
    if getattr(args, "only_seg", False):
        total, vals = stage1_loss(logits, inputs["pcd_label_torch"], None, None, None, None, None, None, None, None, 0, weights, only_seg=True)
        return {"sem_seg_loss": vals[0], "total_loss": total}
    if torch.is_grad_enabled():
        for k in ("PCACoeff", "garment_template_vertices", "Tpose_smpl_vertices_torch", "Tpose_smpl_root_joints_torch"):
            if inputs[k].requires_grad:
                raise NotImplementedError(f"temporal_loss_PCA: inputs['{k}'] requires grad -- only the logits, the PCA coefficients and the T-pose "
                                          "garment are differentiated")
    with torch.no_grad():
        body_v = inputs["Tpose_smpl_vertices_torch"].to(dev).reshape(B, -1, 3).float().contiguous()
        root = inputs["Tpose_smpl_root_joints_torch"].to(dev).reshape(B, 3).float()
        assert body_model.faces.shape[1] == 3 and body_v.shape[1] >= 3, "body needs triangle faces and >= 3 vertices"
        key = id(body_model)
        if key not in _vf:
            fid, vid = mesh_utils.calc_body_mesh_info(body_model)
            _vf.clear()
            _vf[key] = (fid.cuda(), vid.cuda(), torch.from_numpy(np.asarray(body_model.faces).astype(np.int64)).cuda())
        fid, vid, faces = _vf[key]
        body_vn = mesh_utils.compute_vnorms(body_v, faces, vid, fid)
    coeff = output_dict["garment_PCA_coeff"].reshape(B, -1)
    pred = output_dict["tpose_garment"].reshape(B, -1, 3)
    total, vals = stage1_loss(logits, inputs["pcd_label_torch"], coeff, inputs["PCACoeff"].reshape(B, -1), pred,
                              inputs["garment_template_vertices"].reshape(B, -1, 3), root, body_v, body_vn, output_dict["garment_f_3"],
                              int(args.batch_size), weights)
    out = {k: vals[i] for i, k in enumerate(STAGE1_VALUES)}
    out["total_loss"] = total
    return out
