"""The temporal garment refinement loop around the hot path -- `PCALBSGarmentUseSegEncoderSeg.forward`'s
ITERATION rounds (modules/mesh_encoder.py:445-486) with the reference's sub-module names
(`body_positional_encoding{0,1,2}`, `garment_positional_encoding{0,1,2}`, `temporal_qkv_{1,2}`,
`lbs_graph_regress{1,2,3}`) so that the corresponding slices of a reference checkpoint load by key.

Per round: 3 body + 3 garment positional encoders (ball query -> grouped [xyz-offset | feature] rows -> Linear-ReLU-Linear
-> max over the samples: ONE fused MFMA stack launch each, written straight into its 32-column slot of the GCN input),
temporal attention over the T frames of a clip (rounds 1, 2), four GCN layers, residual update of the vertices.
Frame sharding: pass `group` + `frame_ids`; the only exchange is the all-gather inside dist.temporal_attention.
Inference by default.  Opt-in training (tuning.Tuning.refine_autograd, environment G4D_REFINE_AUTOGRAD): under grad the head builds an
autograd graph whose forward launches are the inference route's (the same bits) and whose backward runs csrc/pos_encode_grad.hip,
csrc/attention_grad.hip and the GCN kernels of csrc/gcn_grad.hip; frame-sharded runs stay inference-only.  SURVEY.md section 8f rank 1 -- parity unpinned (mesh_encoder.py cannot be imported here), checked
against oracle/refine_oracle.py."""
import torch
import torch.nn as nn

from . import _cache
from . import _lib
from . import dist as gdist
from . import fused
from . import grad_ops
from . import tuning as _tuning
from .tuning import current as _T
from .gcn import GraphConvolution, gcn_stack_forward


# (USE_PE_KERNEL -> tuning.Tuning.use_pe_kernel) tests flip this to cover the generic fused-stack route


def _pack_linear_mlp(seq):
    """nn.Sequential(Linear, ReLU, Linear) -> packed layers (cached on the module)."""
    def build():
        layers, mods = [], list(seq.children())
        for i, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                dev = m.weight.device
                bias = m.bias.detach().float() if m.bias is not None else torch.zeros(m.out_features, device=dev)
                layers.append(fused.PackedLayer(m.weight.detach().float(), torch.ones(m.out_features, device=dev), bias, relu=relu))
        return layers

    return _cache.packed(seq, "packed", seq.parameters(), build)


def _split_first_linear(seq):
    """Sequential(Linear(3+C, H), ReLU, Linear(H, H)) -> (table layer C -> H with the bias, stack [3+H -> H (ReLU), H -> H]).
    The first Linear is linear in its input, so  W [x_j - q ; f_j] + b = Wx (x_j - q) + (Wf f_j + b): the feature part
    G_j = Wf f_j + b depends on the SOURCE point only and is computed once per level (N_i rows) instead of once per
    (query, sample) pair (Vg * S rows), and the grouped row shrinks from 3 + C (up to 387) to 3 + H = 35 columns
    [x_j - q ; G_j] against the weight [Wx | I].  The coordinate difference is still formed first, in fp32, as the
    reference does; only the summation order of the feature dot product changes."""
    def build():
        lin0, lin2 = seq[0], seq[2]
        H, dev = lin0.out_features, lin0.weight.device
        W = lin0.weight.detach().float()
        ones, zeros = torch.ones(H, device=dev), torch.zeros(H, device=dev)
        table = fused.PackedLayer(W[:, 3:].contiguous(), ones, lin0.bias.detach().float(), relu=False)
        first = fused.PackedLayer(torch.cat([W[:, :3], torch.eye(H, device=dev)], 1), ones, zeros, relu=True)
        second = fused.PackedLayer(lin2.weight.detach().float(), torch.ones(lin2.out_features, device=dev), lin2.bias.detach().float(),
                                   relu=False)
        return table, [first, second]

    return _cache.packed(seq, "split", seq.parameters(), build)


def _pe_stack(layers, idx, nsample, xyz, new_xyz, feats_pm, out, col0):
    """grouped [x_j - q ; feats_j] rows -> layers -> max over the samples, into out[..., col0:col0+Cout]."""
    F_, N, _ = xyz.shape
    Vg = new_xyz.shape[1]
    C = feats_pm.shape[2]
    rows = F_ * Vg * nsample
    grp = (N, Vg, C, 1, xyz, new_xyz, feats_pm, idx)
    if fused.stack_fits(layers, 1, nsample, rows=rows):
        fused.mlp_stack(1, rows, 3 + C, layers, out, col0=col0, pool=1, S=nsample, group=grp)
    else:  # other window sizes: un-pooled stack output, then the row-pool kernel
        tmp = torch.empty((rows, layers[-1].Cout), dtype=torch.float32, device=xyz.device)
        fused.mlp_stack(1, rows, 3 + C, layers, tmp, pool=0, S=nsample, group=grp)
        fused._pool_rows(tmp, F_ * Vg, nsample, out, col0, True)


def _pe_kernel_weights(seq, n_in):
    """Operands of g4d_pos_encode_f32 for Sequential(Linear(3+C, 32), ReLU, Linear(32, 32)): W1 restricted to the first
    n_in input columns (row-major), b1, the second Linear in MFMA fragment order, b2.  None when the shapes differ."""
    if not (len(seq) == 3 and isinstance(seq[0], nn.Linear) and isinstance(seq[1], nn.ReLU) and isinstance(seq[2], nn.Linear)
            and seq[0].out_features == 32 and seq[2].in_features == 32 and seq[2].out_features == 32 and seq[2].bias is not None
            and seq[0].bias is not None):
        return None
    def build():
        W1 = seq[0].weight.detach().float()[:, :n_in].contiguous()
        second = fused.PackedLayer(seq[2].weight.detach().float(), torch.ones(32, device=W1.device), seq[2].bias.detach().float(), relu=False)
        return W1, seq[0].bias.detach().float().contiguous(), second.Wf, seq[2].bias.detach().float().contiguous()

    return _cache.packed(seq, "pe", seq.parameters(), build, extra=n_in)


def positional_encoding(mlp, radius, nsample, xyz, new_xyz, feats_pm, out, col0, idx=None, table=None, _kernel_only=False):
    """QueryAndGroup(radius, nsample, use_xyz=True) -> mlp -> max over samples, into out[..., col0:col0+Cout].
    xyz (F,N,3) cloud, new_xyz (F,Vg,3) queries, feats_pm (F,N,C) point-major.  idx: precomputed ball query;
    table: precomputed per-source-point first-layer feature part (see _split_first_linear) for wide features.
    The reference's shapes (hidden = out = 32, nsample a power of two <= 64, C <= 5 or a table) run on the dedicated
    wave-autonomous kernel (csrc/pos_encode.hip); anything else on the generic fused stack -- also a frame of fewer than 64 grouped rows
    (Vg * nsample < 64: a wave's 64-row chunk would span more than two frames, the launcher refuses it)."""
    if idx is None:
        idx = fused.ball_query_msg([radius], [nsample], xyz, new_xyz)[0]
    F_, N, _ = xyz.shape
    Vg = new_xyz.shape[1]
    C = feats_pm.shape[2]
    n_extra = 0 if table is not None else C
    w = _pe_kernel_weights(mlp, 3 + n_extra) if ((_T().use_pe_kernel or _kernel_only) and nsample in (4, 8, 16, 32, 64) and n_extra <= 5
                                                 and Vg * nsample >= 64) else None
    assert w is not None or not _kernel_only
    if w is not None:
        W1, b1, W2f, b2 = w
        _lib.call("g4d_pos_encode_f32", F_, N, Vg, nsample, n_extra, xyz.data_ptr(), new_xyz.data_ptr(),
                  feats_pm.data_ptr() if n_extra else 0, table.data_ptr() if table is not None else 0, idx.data_ptr(), W1.data_ptr(),
                  0 if table is not None else b1.data_ptr(), W2f.data_ptr(), b2.data_ptr(), out.data_ptr(), out.shape[-1], col0, _lib.stream_ptr())
    elif table is not None:
        _pe_stack(_split_first_linear(mlp)[1], idx, nsample, xyz, new_xyz, table, out, col0)
    else:
        _pe_stack(_pack_linear_mlp(mlp), idx, nsample, xyz, new_xyz, feats_pm, out, col0)


def feature_table(mlp, feats_pm):
    """G = Wf f + b for every source point: (F,N,C) -> (F,N,H).  Constant over the refinement rounds."""
    t = _split_first_linear(mlp)[0]
    F_, N, C = feats_pm.shape
    return fused.linear(feats_pm.reshape(F_ * N, C), t).view(F_, N, -1)


# ---------------------------------------------------------------------------------------------------------------- training route (opt-in)
class _FeatureTableFn(torch.autograd.Function):
    """G = Wf f + b1 per source point (feature_table: the same launch and bits); backward over kernels that exist: dWf = dG^T f
    (g4d_gemm_tn_f32), db1 = column sums of dG (g4d_col_sum_rows_f32), df = dG Wf (g4d_linear_f32)."""

    @staticmethod
    def forward(ctx, feats, Wf, b1, mlp):
        ctx.save_for_backward(feats, Wf)
        return feature_table(mlp, feats)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dG):
        feats, Wf = ctx.saved_tensors
        F_, N, C = feats.shape
        rows, H = F_ * N, Wf.shape[0]
        dG = dG.contiguous().float()
        df = dWf = db = None
        if ctx.needs_input_grad[0]:
            df = grad_ops.linear_t(dG.view(rows, H), Wf).view(F_, N, C)
        if ctx.needs_input_grad[1]:
            dWf = grad_ops.gemm_tn(rows, C, C, H, feats, dG).t().to(Wf.dtype)
        if ctx.needs_input_grad[2]:
            db = grad_ops.col_sum(rows, H, dG)
        return df, dWf, db, None


class _PosEncodeFn(torch.autograd.Function):
    """One positional encoder on g4d_pos_encode_f32 (the inference launch) with g4d_pos_encode_grad_f32 as its backward.  W1 is the part of
    the first Linear the kernel contracts ((32, 3 + n_extra); with a table its xyz columns), b1 None with a table.  The ball-query
    indices are constants of the graph, as in the reference's QueryAndGroup."""

    @staticmethod
    def forward(ctx, new_xyz, xyz, extra, table, W1, b1, W2, b2, mlp, idx, nsample):
        F_, N, _ = xyz.shape
        Vg = new_xyz.shape[1]
        n_extra = 0 if table is not None else (0 if extra is None else extra.shape[2])
        out = torch.empty((F_, Vg, 32), dtype=torch.float32, device=xyz.device)
        positional_encoding(mlp, None, nsample, xyz, new_xyz, extra if extra is not None else xyz[..., :0], out, 0, idx=idx, table=table, _kernel_only=True)
        ctx.dims = (F_, N, Vg, nsample, n_extra)
        ctx.save_for_backward(new_xyz, xyz, extra, table, idx, W1, W2, b1)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        new_xyz, xyz, extra, table, idx, W1, W2, b1 = ctx.saved_tensors
        F_, N, Vg, S, n_extra = ctx.dims
        dev = xyz.device
        need = ctx.needs_input_grad
        dout, ldg = grad_ops.grad_window(dout, 32)
        W1c, W2c = W1.detach().float().contiguous(), W2.detach().float().contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        d_new = torch.empty((F_, Vg, 3), **f32) if need[0] else None
        d_xyz = torch.zeros((F_, N, 3), **f32) if need[1] else None
        d_extra = torch.zeros((F_, N, n_extra), **f32) if (need[2] and n_extra) else None
        d_table = torch.zeros((F_, N, 32), **f32) if (need[3] and table is not None) else None
        dW1 = torch.empty((32, 3 + n_extra), **f32) if need[4] else None
        db1 = torch.empty(32, **f32) if (need[5] and table is None) else None
        dW2 = torch.empty((32, 32), **f32) if need[6] else None
        db2 = torch.empty(32, **f32) if need[7] else None
        ws = None
        if dW1 is not None or db1 is not None or dW2 is not None or db2 is not None:
            ws = _lib.workspace(_lib.lib().g4d_pos_encode_grad_ws_bytes(F_, Vg, S), dev)
        P = lambda t: 0 if t is None else t.data_ptr()
        b1c = None if table is not None else b1.detach().float().contiguous()   # with a table the bias sits in the table (NULL, as in the forward)
        _lib.call("g4d_pos_encode_grad_f32", F_, N, Vg, S, n_extra, xyz.data_ptr(), new_xyz.data_ptr(), P(extra) if n_extra else 0, P(table),
                  idx.data_ptr(), W1c.data_ptr(), P(b1c), W2c.data_ptr(), dout.data_ptr(), ldg, 0, P(ws), P(dW1), P(db1), P(dW2), P(db2), P(d_new),
                  P(d_xyz), P(d_extra), P(d_table), _lib.stream_ptr())
        return d_new, d_xyz, d_extra, d_table, dW1, db1, dW2, db2, None, None, None


def _positional_encoding_autograd(mlp, nsample, xyz, new_xyz, feats_pm, idx, table):
    """The training route of positional_encoding: returns the (F, Vg, 32) block (the caller concatenates).  Only the dedicated kernel's
    shape domain has a backward."""
    C = feats_pm.shape[2]
    n_extra = 0 if table is not None else C
    ok = nsample in (4, 8, 16, 32, 64) and n_extra <= 5 and _pe_kernel_weights(mlp, 3 + n_extra) is not None and new_xyz.shape[1] * nsample >= 64
    if not ok:
        raise NotImplementedError(f"positional encoder backward: only the dedicated kernel's shapes (hidden = out = 32, nsample in 4|8|16|32|64, "
                                  f"at most 5 extra columns or a table) -- got nsample {nsample}, {C} feature columns, table {table is not None}, "
                                  f"mlp {mlp}")
    lin0, lin2 = mlp[0], mlp[2]
    xyz, new_xyz, feats_pm = xyz.contiguous(), new_xyz.contiguous(), feats_pm.contiguous()
    if table is not None:
        return _PosEncodeFn.apply(new_xyz, xyz, None, table, lin0.weight[:, :3], None, lin2.weight, lin2.bias, mlp, idx, nsample)
    return _PosEncodeFn.apply(new_xyz, xyz, feats_pm if n_extra else None, None, lin0.weight, lin0.bias, lin2.weight, lin2.bias, mlp, idx, nsample)


class GarmentRefinementHead(nn.Module):
    def __init__(self, garment_name="Tshirt", iteration=3, garment_pe_input_dim=(3 + 64, 3 + 32 + 64, 3 + 128 + 256)):
        super().__init__()
        self.iteration = iteration
        self.garment_radius_list = [0.1, 0.2, 0.4]
        self.garment_sample_num_list = [32, 8, 4] if garment_name == "Trousers" else [32, 16, 8]   # mesh_encoder.py:180-189
        self.body_radius_list = [0.1, 0.2, 0.4]
        self.body_sample_num_list = [8, 16, 32]
        self.feat_num = 32
        self.hidden_dim = 128
        self.graph_start_feature_dim = self.feat_num * 6 + 3

        def pe(cin):
            return nn.Sequential(nn.Linear(cin, self.feat_num), nn.ReLU(), nn.Linear(self.feat_num, self.feat_num))

        self.body_positional_encoding0, self.body_positional_encoding1, self.body_positional_encoding2 = pe(6), pe(6), pe(6)
        self.garment_positional_encoding_input_dim = list(garment_pe_input_dim)
        self.garment_positional_encoding0 = pe(garment_pe_input_dim[0])
        self.garment_positional_encoding1 = pe(garment_pe_input_dim[1])
        self.garment_positional_encoding2 = pe(garment_pe_input_dim[2])
        self.temporal_qkv_1 = nn.Linear(self.hidden_dim, self.hidden_dim * 3, bias=False)
        self.temporal_qkv_2 = nn.Linear(self.hidden_dim, self.hidden_dim * 3, bias=False)

        def gcn(first):
            return nn.ModuleList([GraphConvolution(first, self.hidden_dim), GraphConvolution(self.hidden_dim, self.hidden_dim),
                                  GraphConvolution(self.hidden_dim, self.hidden_dim), GraphConvolution(self.hidden_dim, 3)])

        self.lbs_graph_regress1 = gcn(self.graph_start_feature_dim)
        self.lbs_graph_regress2 = gcn(self.graph_start_feature_dim + self.hidden_dim)
        self.lbs_graph_regress3 = gcn(self.graph_start_feature_dim + self.hidden_dim)

    def _stages(self):
        """The sub-modules in the order the rounds use them: body encoders, garment encoders (per level), qkv Linears (rounds 1, 2) and
        regressors (per round)."""
        return ([self.body_positional_encoding0, self.body_positional_encoding1, self.body_positional_encoding2],
                [self.garment_positional_encoding0, self.garment_positional_encoding1, self.garment_positional_encoding2],
                [self.temporal_qkv_1, self.temporal_qkv_2],
                [self.lbs_graph_regress1, self.lbs_graph_regress2, self.lbs_graph_regress3])

    def _round_width(self, it):
        """(width, wpad) of round `it`'s GCN input: 195 / 323 columns, and the row padded to 16 bytes (zero columns) so that the tiled GEMM
        takes the regressor's first contraction."""
        width = self.graph_start_feature_dim + (self.hidden_dim if it > 0 else 0)
        return width, (width + 3) // 4 * 4

    def _qkv(self, lin):
        dev = lin.weight.device
        L = _cache.packed(lin, "packed", [lin.weight], lambda: fused.PackedLayer(
            lin.weight.detach().float(), torch.ones(lin.out_features, device=dev), torch.zeros(lin.out_features, device=dev), relu=False))
        return lambda x: fused.linear(x.reshape(-1, x.shape[-1]).contiguous(), L).view(*x.shape[:-1], -1)

    def forward(self, cur_garment_v, body_v, body_vn, garment_v_list, garment_f_list, adj, nbatch, T, group=None, frame_ids=None,
                clip_range=None):
        """cur_garment_v (F,Vg,3) LBS-posed garment; body_v / body_vn (F,V,3) body vertices / normals; garment_v_list[i] (F,N_i,3)
        and garment_f_list[i] (F,N_i,C_i) POINT-major encoder levels; adj the normalised garment adjacency; F = local frames
        (= nbatch*T without sharding; with sharding pass the process group and the global ids of the local frames).
        Returns the list of refined vertices per round (mesh_encoder.py:485)."""
        if torch.is_grad_enabled() and _T().refine_autograd:
            return self._forward_autograd(cur_garment_v, body_v, body_vn, garment_v_list, garment_f_list, adj, nbatch, T, group)
        assert not torch.is_grad_enabled(), ("GarmentRefinementHead is inference-only: call under torch.no_grad() (or opt in to the backward "
                                             "kernels: tuning.Tuning.refine_autograd / G4D_REFINE_AUTOGRAD=1)")
        body_pe, garm_pe, qkvs, regress = self._stages()
        F_, Vg, _ = cur_garment_v.shape
        dev = cur_garment_v.device
        if frame_ids is None:
            frame_ids = torch.arange(F_, device=dev)
        n_frames = nbatch * T
        cur = cur_garment_v.contiguous()
        outs, lbs_iter_feat = [], []
        pending = None   # all-gather of the previous round's attention features, in flight (frame-sharded runs only)
        # per-source-point first-layer tables of the garment encoders: the garment levels do not change over the rounds
        tables = [feature_table(garm_pe[i], garment_f_list[i].contiguous()) if garment_f_list[i].shape[2] > self.feat_num else None
                  for i in range(3)]
        for it in range(self.iteration):
            width, wpad = self._round_width(it)
            feat = torch.empty((F_, Vg, wpad), dtype=torch.float32, device=dev)
            if wpad > width:
                feat[..., width:] = 0
            feat[..., :3] = cur                                                      # cur_positional_encoding (:465)
            col = 3
            body_idx = fused.ball_query_msg(self.body_radius_list, self.body_sample_num_list, body_v, cur, coherent=True)   # one pass, 3 radii
            for i in range(3):                                                       # :452-457
                positional_encoding(body_pe[i], self.body_radius_list[i], self.body_sample_num_list[i], body_v, cur, body_vn, feat, col,
                                    idx=body_idx[i])
                col += self.feat_num
            for i in range(3):                                                       # :459-464
                positional_encoding(garm_pe[i], self.garment_radius_list[i], self.garment_sample_num_list[i], garment_v_list[i], cur,
                                    garment_f_list[i], feat, col, table=tables[i])
                col += self.feat_num
            if it > 0:                                                               # :467-476
                gdist.temporal_attention(lbs_iter_feat[-2], frame_ids, n_frames, T, self._qkv(qkvs[it - 1]), group, out=feat, col0=col,
                                         clip_range=clip_range, gathered=pending)
                pending = None
            # :477-481 -- four chained GraphConvolutions; only the third one's output (the next round's attention input) and the
            # last one's are kept, the rest never leaves the fused aggregate + contract launches (gcn.gcn_stack_forward)
            hs = gcn_stack_forward(regress[it], feat, adj, relu_last=False, keep=(2,), in_width=width)
            lbs_iter_feat += hs
            h = hs[-1]
            if it + 1 < self.iteration and gdist.resolve_group(group) is not None:
                # the next round's attention needs this tensor from every rank: start the all-gather now, it overlaps the next
                # round's six ball queries + positional encoders, which do not depend on it
                pending = gdist.allgather_frames_async(hs[2], n_frames, group)
            cur = (cur + h).contiguous()                                             # :482-483
            outs.append(cur)
        return outs

    def _forward_autograd(self, cur_garment_v, body_v, body_vn, garment_v_list, garment_f_list, adj, nbatch, T, group):
        """The training route (tuning.Tuning.refine_autograd): the same launches as the inference route -- so every round's output has the same
        bits -- inside torch.autograd.Functions, the column slots of the GCN input replaced by one torch.cat per round.  Gradients reach every
        parameter of the head, cur_garment_v (direct copy, residual and every x_j - q) and garment_v_list[i] / garment_f_list[i] when they
        require grad; body_v / body_vn are constants; the ball-query indices are constants of the graph (the reference's QueryAndGroup)."""
        if group is not None and group is not False:
            raise NotImplementedError("GarmentRefinementHead: frame-sharded runs (group=...) are inference-only; train with whole clips per rank")
        body_pe, garm_pe, qkvs, regress = self._stages()
        F_, Vg, _ = cur_garment_v.shape
        dev = cur_garment_v.device
        n_frames = nbatch * T
        assert F_ == n_frames, "the training route takes whole clips: F = nbatch * T frames"
        frame_ids = torch.arange(F_, device=dev)
        body_v, body_vn = body_v.detach().contiguous(), body_vn.detach().contiguous()
        gv = [v.contiguous() for v in garment_v_list]
        gf = [f.contiguous() for f in garment_f_list]
        cur = cur_garment_v.contiguous()
        outs, lbs_iter_feat = [], []
        tables = []
        for i in range(3):
            if gf[i].shape[2] > self.feat_num:
                lin0 = garm_pe[i][0]
                tables.append(_FeatureTableFn.apply(gf[i], lin0.weight[:, 3:], lin0.bias, garm_pe[i]))
            else:
                tables.append(None)
        with _tuning.use(_T().replace(gcn_autograd=True)):
            for it in range(self.iteration):
                width, wpad = self._round_width(it)
                with torch.no_grad():
                    body_idx = fused.ball_query_msg(self.body_radius_list, self.body_sample_num_list, body_v, cur.detach(), coherent=True)
                    garm_idx = [fused.ball_query_msg([self.garment_radius_list[i]], [self.garment_sample_num_list[i]], gv[i].detach(), cur.detach())[0]
                                for i in range(3)]
                blocks = [cur]
                for i in range(3):
                    blocks.append(_positional_encoding_autograd(body_pe[i], self.body_sample_num_list[i], body_v, cur, body_vn, body_idx[i], None))
                for i in range(3):
                    blocks.append(_positional_encoding_autograd(garm_pe[i], self.garment_sample_num_list[i], gv[i], cur, gf[i], garm_idx[i], tables[i]))
                if it > 0:
                    blocks.append(gdist.temporal_attention(lbs_iter_feat[-2], frame_ids, n_frames, T, self._qkv(qkvs[it - 1]), None,
                                                           qkv_linear=qkvs[it - 1]))
                if wpad > width:
                    blocks.append(torch.zeros((F_, Vg, wpad - width), dtype=torch.float32, device=dev))
                feat = torch.cat(blocks, dim=-1)
                hs = gcn_stack_forward(regress[it], feat, adj, relu_last=False, keep=(2,), in_width=width)
                lbs_iter_feat += hs
                cur = (cur + hs[-1]).contiguous()
                outs.append(cur)
        return outs
