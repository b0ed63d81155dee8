"""Launch helpers the backward passes share (gcn._GCNLayerFn, refine._FeatureTableFn / _PosEncodeFn, dist._TemporalAttentionFn,
garment_lbs._MGNSkinFn, mesh_encoder._LinearFn): each wraps
one kernel with its full argument set and sizes its workspace, so that kernel has one Python call site."""
import torch

from . import _lib
from . import fused


def grad_window(g, width):
    """A cotangent (F, V, width) as (tensor, leading dimension): the column window of a wider row-major buffer (what the backward of
    torch.cat hands over) is read in place through its row stride; anything else is made contiguous."""
    if g.dtype != torch.float32:
        g = g.float()
    F_, V, _ = g.shape
    if g.stride(2) == 1 and g.stride(1) >= width and g.stride(0) == V * g.stride(1):
        return g, g.stride(1)
    return g.contiguous(), width


def col_sum(rows, c, g, mask=None):
    """Column sums (c,) of the (rows, c) matrix g, of the entries where mask > 0 when a mask (the output of a fused ReLU) is given:
    g4d_col_sum_rows_f32."""
    out = torch.empty(c, dtype=torch.float32, device=g.device)
    ws = _lib.workspace(_lib.lib().g4d_col_sum_rows_ws_bytes(rows, c), g.device)
    _lib.call("g4d_col_sum_rows_f32", rows, c, g.data_ptr(), 0 if mask is None else mask.data_ptr(), ws.data_ptr(), out.data_ptr(),
              _lib.stream_ptr())
    return out


def gemm_tn(rows, fin, ldx, cout, x, ds):
    """X^T dS (fin, cout) over `rows` rows, X being the first fin columns of rows ldx >= fin apart: g4d_gemm_tn_f32, slice partials added
    in a fixed order."""
    dw = torch.empty((fin, cout), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(_lib.lib().g4d_gemm_tn_ws_bytes(rows, fin, cout), x.device)
    _lib.call("g4d_gemm_tn_f32", rows, fin, ldx, cout, x.data_ptr(), ds.data_ptr(), ws.data_ptr(), dw.data_ptr(), _lib.stream_ptr())
    return dw


def mgn_skin_grad(clips, frames_per_clip, idx, W, inv_A, A, d_posed, d_stage1=None):
    """d garment (F, Vg, 3) of lbs_garment_MGN for the fixed nearest index idx (F, Vg) int32 -- M_inv^T (M^T d_posed + d_stage1) with the
    forward's blends recomputed: g4d_mgn_skin_grad_f32.  d_stage1 None: zero."""
    F_, V, J = W.shape
    Vg = idx.shape[1]
    out = torch.empty((F_, Vg, 3), dtype=torch.float32, device=W.device)
    _lib.call("g4d_mgn_skin_grad_f32", clips, frames_per_clip, Vg, V, J, idx.data_ptr(), W.data_ptr(), inv_A.data_ptr(), A.data_ptr(),
              d_posed.data_ptr(), 0 if d_stage1 is None else d_stage1.data_ptr(), out.data_ptr(), _lib.stream_ptr())
    return out


def garment_skin_grad(clips, frames_per_clip, W, A, verts, d_out, d_add=None, want_verts=True, want_W=True):
    """The adjoint of lbs.skin() in the garment's form (g4d_garment_skin_grad_f32): W (clips * frames_per_clip, Vg, J) or (clips, Vg, J) = one table
    per clip, A (frames, J, 4, 4), verts (clips, Vg, 3) shared by a clip's frames, d_out (frames, Vg, 3) -> (d_verts (clips, Vg, 3) = d_add + the
    sum over the clip's frames, d_W in W's shape); either is None when not wanted."""
    _lib.skin_lib()
    Vg, J = W.shape[1], W.shape[2]
    per_clip = int(W.shape[0] == clips and frames_per_clip > 1)
    d_verts = torch.empty((clips, Vg, 3), dtype=torch.float32, device=W.device) if want_verts else None
    d_W = torch.empty_like(W) if want_W else None
    _lib.call("g4d_garment_skin_grad_f32", clips, frames_per_clip, Vg, J, W.data_ptr(), per_clip, A.data_ptr(), verts.data_ptr(), d_out.data_ptr(),
              0 if d_add is None else d_add.data_ptr(), 0 if d_verts is None else d_verts.data_ptr(), 0 if d_W is None else d_W.data_ptr(),
              _lib.stream_ptr())
    return d_verts, d_W


def knn_blend_grad(W, frames_per_clip, idx32, dists, k, d_blend, pts, ref, d_add=None):
    """The adjoint of the inverse-distance blend carried on to the query points (g4d_knn_blend_grad_f32): W (F, V, J), idx32 / dists
    (F / frames_per_clip, Vg, ldk) of which the first k entries of a row are used, d_blend (F, Vg, J), pts (clips, Vg, 3), ref (clips, V, 3)
    -> d_pts (clips, Vg, 3) = d_add + d g."""
    _lib.skin_lib()
    F_, V, J = W.shape
    clips, Vg, ldk = idx32.shape
    out = torch.empty((clips, Vg, 3), dtype=torch.float32, device=W.device)
    _lib.call("g4d_knn_blend_grad_f32", F_, frames_per_clip, Vg, V, int(k), ldk, J, W.data_ptr(), idx32.data_ptr(), dists.data_ptr(), d_blend.data_ptr(),
              pts.data_ptr(), ref.data_ptr(), 0 if d_add is None else d_add.data_ptr(), out.data_ptr(), _lib.stream_ptr())
    return out


def linear_t(ds2d, weight):
    """dS . W for a Linear weight W (Cout, Cin): g4d_linear_f32 with W^T as the packed (Cin x Cout-deep) layer."""
    cin = weight.shape[1]
    with torch.no_grad():
        L = fused.PackedLayer(weight.detach().float().t().contiguous(), torch.ones(cin, device=weight.device),
                              torch.zeros(cin, device=weight.device), relu=False)
    return fused.linear(ds2d, L)


def bn_stats(rows, c, y, ldy):
    """(mean, biased variance), each (c,), over the rows of the first c columns of y (rows ldy >= c apart): g4d_bn_stats_f32, two passes, slice
    partials added in a fixed order."""
    mean = torch.empty(c, dtype=torch.float32, device=y.device)
    var = torch.empty(c, dtype=torch.float32, device=y.device)
    ws = _lib.workspace(_lib.lib().g4d_bn_stats_ws_bytes(rows, c), y.device)
    _lib.call("g4d_bn_stats_f32", rows, c, y.data_ptr(), ldy, ws.data_ptr(), mean.data_ptr(), var.data_ptr(), _lib.stream_ptr())
    return mean, var


def bn_act(rows, c, y, ldy, mean, var, eps, gamma, beta, relu, out=None, ldo=None):
    """act(gamma * (y - mean) / sqrt(var + eps) + beta), (rows, c): g4d_bn_act_f32.  gamma / beta None: 1 / 0."""
    if out is None:
        out, ldo = torch.empty((rows, c), dtype=torch.float32, device=y.device), c
    _lib.call("g4d_bn_act_f32", rows, c, y.data_ptr(), ldy, mean.data_ptr(), var.data_ptr(), float(eps), fused._ptr(gamma), fused._ptr(beta), int(relu),
              out.data_ptr(), ldo, _lib.stream_ptr())
    return out


def bn_act_grad_reduce(rows, c, dout, ldg, y, ldy, mean, var, eps, gamma, beta, relu):
    """(dgamma, dbeta) = (sum G * xhat, sum G) with G = dout where the activation passed: g4d_bn_act_grad_reduce_f32 (mask and xhat recomputed from y)."""
    dgamma = torch.empty(c, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=y.device)
    ws = _lib.workspace(_lib.lib().g4d_bn_act_grad_reduce_ws_bytes(rows, c), y.device)
    _lib.call("g4d_bn_act_grad_reduce_f32", rows, c, dout.data_ptr(), ldg, y.data_ptr(), ldy, mean.data_ptr(), var.data_ptr(), float(eps),
              fused._ptr(gamma), fused._ptr(beta), int(relu), ws.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _lib.stream_ptr())
    return dgamma, dbeta


def bn_act_grad(rows, c, dout, ldg, y, ldy, mean, var, eps, gamma, beta, relu, batch_stats, dgamma=None, dbeta=None):
    """dY (rows, c) of act(BatchNorm(Y)): g4d_bn_act_grad_f32.  batch_stats False (running statistics): the two mean terms are dropped and
    dgamma / dbeta are not read."""
    dy = torch.empty((rows, c), dtype=torch.float32, device=y.device)
    _lib.call("g4d_bn_act_grad_f32", rows, c, dout.data_ptr(), ldg, y.data_ptr(), ldy, mean.data_ptr(), var.data_ptr(), float(eps), fused._ptr(gamma),
              fused._ptr(beta), int(relu), int(batch_stats), fused._ptr(dgamma), fused._ptr(dbeta), dy.data_ptr(), c, _lib.stream_ptr())
    return dy


def pool_rows_max_grad(groups, S, c, x, ldx, dpooled, ldp, col0=0):
    """dX (groups * S, c) of the row max-pool: dpooled at the first row of each group attaining the maximum, 0 elsewhere: g4d_pool_rows_max_grad_f32."""
    dx = torch.empty((groups * S, c), dtype=torch.float32, device=x.device)
    _lib.call("g4d_pool_rows_max_grad_f32", groups, S, c, x.data_ptr(), ldx, dpooled.data_ptr(), ldp, col0, dx.data_ptr(), _lib.stream_ptr())
    return dx
