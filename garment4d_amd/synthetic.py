"""Seeded synthetic inputs shaped like the reference's data.

There is no CLOTH3D data, SMPL model file or checkpoint in this environment, so tests, the
golden-fixture generator and bench.py all draw from these generators (numpy Generator/PCG64,
explicit seeds).  numpy only -- no torch, no HIP.
"""
import numpy as np

F32 = np.float32

# SMPL kinematic tree (24 joints), as in the SMPL model files the reference loads
# (smplx/smplx/body_models.py:49-251 reads `kintree_table`); parents[0] = -1.
SMPL_PARENTS = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21],
                        dtype=np.int64)


def unit_cloud(B, N, seed=0):
    """xyz ~ U[0,1)^3, fp32, (B,N,3)."""
    return np.random.default_rng(seed).random((B, N, 3), dtype=F32)


def body_like_cloud(B, N, seed=0, dup_frac=0.2, zero_frac=0.1):
    """Tie-heavy cloud: points on a 1.7 x 0.5 x 0.3 ellipsoid shell (shifted into [0,1]^3-ish),
    a fraction of exact duplicates (the reference up-samples with duplicates,
    utils/dataloader.py:36-44) and a zero-padded tail (modules/mesh_encoder.py:119-124)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((B, N, 3)).astype(F32)
    v /= np.linalg.norm(v, axis=-1, keepdims=True).astype(F32) + F32(1e-12)
    v = v * np.array([0.25, 0.85, 0.15], dtype=F32) + np.array([0.5, 0.9, 0.5], dtype=F32)
    v = v.astype(F32)
    nd = int(N * dup_frac)
    nz = int(N * zero_frac)
    if nd > 0:
        src = rng.integers(0, max(N - nd - nz, 1), size=(B, nd))
        for b in range(B):
            v[b, N - nd - nz:N - nz] = v[b, src[b]]
    if nz > 0:
        v[:, N - nz:] = 0
    return np.ascontiguousarray(v)


def shell_cloud(B, N, seed=0, R=0.5, centre=0.0):
    """Rounding-adversarial cloud: point 0 sits at `centre`, every other point at distance R from it up to fp32 rounding
    (random directions on a sphere).  The squared distances to point 0 then agree to within a few ulps, so WHICH point FPS
    picks, which points a radius-R ball holds and the order of a 3-NN are decided by how the distance expression is rounded --
    the inputs on which the contraction modes of include/g4d.h (fused vs un-fused multiply-adds) give different indices."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((B, N, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    v = (d * R + centre).astype(F32)
    v[:, 0] = centre
    return np.ascontiguousarray(v)


def smpl_like_params(V=6890, J=24, num_betas=10, seed=0):
    """SMPL-shaped random model parameters:
    v_template (V,3), shapedirs (V,3,nb), posedirs ((J-1)*9, V*3), J_regressor (J,V) row-normalised
    sparse-ish positives, parents (J,), lbs_weights (V,J) row-normalised sparse-ish positives."""
    rng = np.random.default_rng(seed)
    v_template = (rng.standard_normal((V, 3)) * np.array([0.25, 0.6, 0.15])).astype(F32)
    shapedirs = (rng.standard_normal((V, 3, num_betas)) * 0.01).astype(F32)
    posedirs = (rng.standard_normal(((J - 1) * 9, V * 3)) * 0.001).astype(F32)
    jr = rng.random((J, V)).astype(F32)
    jr *= (rng.random((J, V)) < min(1.0, 40.0 / V)).astype(F32)
    jr[:, 0] += F32(1e-3)
    J_regressor = (jr / jr.sum(1, keepdims=True)).astype(F32)
    w = rng.random((V, J)).astype(F32) ** 4
    keep = rng.random((V, J)) < (4.0 / J)
    w = w * keep
    w[np.arange(V), rng.integers(0, J, size=V)] += F32(0.5)
    lbs_weights = (w / w.sum(1, keepdims=True)).astype(F32)
    if J == 24:
        parents = SMPL_PARENTS.copy()
    else:
        parents = np.array([-1] + [int(rng.integers(0, i)) for i in range(1, J)], dtype=np.int64)
    return dict(v_template=v_template, shapedirs=shapedirs, posedirs=posedirs, J_regressor=J_regressor,
                parents=parents, lbs_weights=lbs_weights)


def smpl_data_struct(P, faces):
    """SMPL .pkl-shaped dict (the fields smplx/smplx/body_models.py:133-270 reads) from smpl_like_params output."""
    V = P["v_template"].shape[0]
    kin = np.stack([P["parents"].astype(np.int64), np.arange(P["parents"].shape[0], dtype=np.int64)])
    return dict(shapedirs=P["shapedirs"], f=faces, v_template=P["v_template"], J_regressor=P["J_regressor"],
                posedirs=np.ascontiguousarray(P["posedirs"].T).reshape(V, 3, -1), kintree_table=kin, weights=P["lbs_weights"])


def smpl_like_pose(B, J=24, num_betas=10, seed=1):
    """betas ~ N(0,1) (B,nb); axis-angle pose ~ N(0,0.2^2) (B,J*3)."""
    rng = np.random.default_rng(seed)
    betas = rng.standard_normal((B, num_betas)).astype(F32)
    pose = (rng.standard_normal((B, J * 3)) * 0.2).astype(F32)
    return betas, pose


def quad_cylinder(rows, cols):
    """A closed-around quad cylinder: vertices (rows*cols,3), faces (.,4) int32 -- stands in for
    the garment template mesh (`remesh_cylinder_f`, modules/mesh_encoder.py:286)."""
    th = np.linspace(0, 2 * np.pi, cols, endpoint=False)
    h = np.linspace(0, 1, rows)
    verts = np.stack([np.repeat(np.cos(th)[None], rows, 0) * 0.2, np.repeat(h[:, None], cols, 1),
                      np.repeat(np.sin(th)[None], rows, 0) * 0.2], axis=-1).reshape(-1, 3).astype(F32)
    faces = []
    for r in range(rows - 1):
        for c in range(cols):
            a = r * cols + c
            b = r * cols + (c + 1) % cols
            faces.append([a, b, b + cols, a + cols])
    return verts, np.asarray(faces, dtype=np.int32)


def garment_scene(nbatch, T, N, body_rc=(25, 28), garment_rc=(12, 16), pca_dim=64, seed=0):
    """A synthetic stand-in for one batch of the reference's data loader (utils/dataloader.py:186-300) plus the on-disk
    assets of the model constructor (PCA basis pickle, garment template OBJ, SMPL body) -- none of which exist here.
    Body = triangulated quad cylinder (V = rows*cols vertices), garment template = a wider quad cylinder (Vg vertices).
    Returns dict(x (nbatch,T,N,3), batch {reference keys}, body {parents, faces, J_regressor, v_template},
    pca {components, mean, explained, ss_scale}, template (verts, quad faces)); all numpy."""
    rng = np.random.default_rng(seed)
    bv, bq = quad_cylinder(*body_rc)
    bv = (bv * np.array([0.75, 0.7, 0.5], dtype=F32) + np.array([0, -0.35, 0], dtype=F32)).astype(F32)
    V = bv.shape[0]
    faces = np.concatenate([bq[:, [0, 1, 2]], bq[:, [0, 2, 3]]], 0).astype(np.int64)
    P = smpl_like_params(V=V, J=24, seed=seed + 1)
    gv, gq = quad_cylinder(*garment_rc)
    gv = (gv * np.array([1.0, 0.45, 0.7], dtype=F32) + np.array([0, -0.2, 0], dtype=F32)).astype(F32)
    Vg = gv.shape[0]
    pca = dict(components=(rng.standard_normal((pca_dim + 8, Vg * 3)) * 0.002).astype(F32), mean=gv.reshape(-1).copy(),
               explained=rng.random(pca_dim + 8), ss_scale=np.ones(Vg * 3) * 1.0)
    root = (rng.standard_normal((nbatch, 1, 3)) * 0.01).astype(F32)
    shape_off = (rng.standard_normal((nbatch, 1, V, 3)) * 0.003).astype(F32)
    tpose = (bv[None, None] + shape_off).astype(F32)                                   # (nbatch,1,V,3)
    zeropose = np.repeat(tpose, T, 1).astype(F32)                                      # (nbatch,T,V,3)
    pose = (rng.standard_normal((nbatch, T, 72)) * 0.1).astype(F32)
    drift = np.cumsum(rng.standard_normal((nbatch, T, 1, 3)) * 0.004, axis=1).astype(F32)
    smpl_v = (zeropose + drift + rng.standard_normal((nbatch, T, V, 3)).astype(F32) * 0.001).astype(F32)
    # the scan: N points, ~55 % on the body, the rest on the (posed-ish) garment, jittered
    nb = int(N * 0.55)
    x = np.empty((nbatch, T, N, 3), F32)
    for b in range(nbatch):
        for t in range(T):
            bi = rng.integers(0, V, nb)
            gi = rng.integers(0, Vg, N - nb)
            pts = np.concatenate([smpl_v[b, t, bi], gv[gi] + drift[b, t]], 0)
            x[b, t] = pts[rng.permutation(N)] + rng.standard_normal((N, 3)).astype(F32) * 0.004
    batch = {
        "smpl_vertices_torch": smpl_v,
        "Tpose_smpl_vertices_torch": tpose,
        "Tpose_smpl_root_joints_torch": root,
        "zeropose_smpl_vertices_torch": zeropose,
        "pose_torch": pose,
        "T_J_regressor": np.ascontiguousarray(np.broadcast_to(P["J_regressor"][None, None], (nbatch, T) + P["J_regressor"].shape)),
        "T_lbs_weights": np.ascontiguousarray(np.broadcast_to(P["lbs_weights"][None, None], (nbatch, T) + P["lbs_weights"].shape)),
    }
    body = dict(parents=P["parents"], faces=faces, J_regressor=P["J_regressor"], v_template=bv)
    return dict(x=x, batch=batch, body=body, pca=pca, template=(gv, gq))


def refine_state_dict(seed=0, feat=32, hidden=128, garment_in=(67, 99, 387)):
    """Seeded weights under the reference's state-dict names for PCALBSGarmentUseSegEncoderSeg (modules/mesh_encoder.py:201-284):
    six positional encoders (Linear in->32, Linear 32->32), two bias-free temporal q/k/v Linears, three 4-layer GCN regressors
    (195 | 323 -> 128 -> 128 -> 128 -> 3; GraphConvolution stores weight as (in, out), modules/pygcn/layers.py:19).  numpy, fp32."""
    rng = np.random.default_rng(seed)
    sd = {}

    def uni(shape, bound):
        return ((rng.random(shape) * 2 - 1) * bound).astype(F32)
    for i in range(3):
        for name, cin in (("body_positional_encoding%d" % i, 6), ("garment_positional_encoding%d" % i, garment_in[i])):
            sd[name + ".0.weight"] = uni((feat, cin), 1.0 / np.sqrt(cin))
            sd[name + ".0.bias"] = uni((feat,), 1.0 / np.sqrt(cin))
            sd[name + ".2.weight"] = uni((feat, feat), 1.0 / np.sqrt(feat))
            sd[name + ".2.bias"] = uni((feat,), 1.0 / np.sqrt(feat))
    for i in (1, 2):
        sd["temporal_qkv_%d.weight" % i] = uni((3 * hidden, hidden), 0.3 / np.sqrt(hidden))
    start = 6 * feat + 3
    for r in range(3):
        dims = [start + (hidden if r > 0 else 0), hidden, hidden, hidden, 3]
        for l in range(4):
            p = "lbs_graph_regress%d.%d" % (r + 1, l)
            sd[p + ".weight"] = uni((dims[l], dims[l + 1]), 0.5 / np.sqrt(dims[l + 1]) if l < 3 else 0.02)
            sd[p + ".bias"] = uni((dims[l + 1],), 0.5 / np.sqrt(dims[l + 1]) if l < 3 else 0.005)
    return sd


def refine_golden_case(seed=70, nbatch=2, T=3):
    """The inputs of tests/golden/refine.npz (written by tests/golden/make_golden_refine.py, which runs the reference's own
    modules/mesh_encoder.py on them): a 700-vertex body cylinder, the 64-vertex quad-cylinder garment template, three garment
    point levels (128 / 48 / 16 points with 64 / 96 / 384 features, as mesh_encoder.py:236-240 expects), per-clip garment
    templates.  Regenerated from the seed on both sides; refine_golden_checksum() guards against generator drift."""
    sc = garment_scene(nbatch, T, 4, garment_rc=(8, 8), seed=seed)
    rng = np.random.default_rng(seed + 7)
    gv, gq = sc["template"]
    Vg = gv.shape[0]
    F_ = nbatch * T
    tpose_garment = (gv[None] + rng.standard_normal((nbatch, Vg, 3)) * 0.004).astype(F32)
    centre = sc["batch"]["smpl_vertices_torch"].reshape(F_, -1, 3).mean(1, keepdims=True) - sc["body"]["v_template"].mean(0)
    lv, lf = [], []
    for n, c in ((128, 64), (48, 96), (16, 384)):
        sel = rng.integers(0, Vg, n)
        lv.append((gv[sel][None] + centre + rng.standard_normal((F_, n, 3)) * 0.03).astype(F32))
        lf.append(rng.standard_normal((F_, n, c)).astype(F32))                      # point-major (F,N_i,C_i)
    return dict(seed=seed, nbatch=nbatch, T=T, Vg=Vg, batch=sc["batch"], body=sc["body"], template_verts=gv, template_faces=gq,
                tpose_garment=tpose_garment, garment_v_list=lv, garment_f_list=lf)


def refine_golden_checksum(case):
    items = [case["tpose_garment"]] + case["garment_v_list"] + case["garment_f_list"] + [v for _, v in sorted(case["batch"].items())]
    items += [v for _, v in sorted(refine_state_dict(seed=case["seed"] + 100).items())]
    return np.array([float(np.asarray(a, dtype=np.float64).sum()) for a in items])


def vertex_normals(verts, faces):
    """Unit vertex normals (F,V,3) float32 of triangle meshes sharing `faces`: unit face normals summed per vertex, re-normalised (float64
    inside).  Only used to PLACE synthetic garments around a body; the product's normals come from its own kernel."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    fn = np.cross(v[:, f[:, 1]] - v[:, f[:, 0]], v[:, f[:, 2]] - v[:, f[:, 0]])
    fn /= np.maximum(np.linalg.norm(fn, axis=-1, keepdims=True), 1e-12)
    vn = np.zeros_like(v)
    for c in range(3):
        for fr in range(v.shape[0]):
            np.add.at(vn[fr], f[:, c], fn[fr])
    vn /= np.maximum(np.linalg.norm(vn, axis=-1, keepdims=True), 1e-12)
    return vn.astype(F32)


def garment_around_body(rng, body_v, body_n, sel, sigma=0.01, jitter=0.002):
    """(F,len(sel),3) float32: the body vertices `sel` moved along their normals by N(0, sigma) plus N(0, jitter) per coordinate -- about half
    of the vertices end up behind the surface, and none sits at rounding distance of it."""
    F_, n = body_v.shape[0], len(sel)
    return (body_v[:, sel] + body_n[:, sel] * rng.normal(0.0, sigma, (F_, n, 1)) + rng.normal(0.0, jitter, (F_, n, 3))).astype(F32)


def stage2_loss_case(seed=170):
    """The inputs of tests/golden/stage2_loss.npz (written by tests/golden/make_golden_stage2_loss.py, which runs the reference's own
    `temporal_loss_PCA_LBS` on them): the body and the 64-vertex quad-cylinder template of refine_golden_case, three leaf rounds and an
    `lbs_pred_garment_v` placed around the body (garment_around_body; garment vertex i follows body vertex sel[i] in every frame), random
    `garment_torch` (near the rounds, relative to the root) and random root joints.  stage2_loss_checksum() guards against generator drift."""
    base = refine_golden_case()
    nbatch, T, Vg = base["nbatch"], base["T"], base["Vg"]
    F_ = nbatch * T
    rng = np.random.default_rng(seed)
    body_v = base["batch"]["smpl_vertices_torch"].reshape(F_, -1, 3)
    body_n = vertex_normals(body_v, base["body"]["faces"])
    sel = rng.permutation(body_v.shape[1])[:Vg]
    rounds = [garment_around_body(rng, body_v, body_n, sel) for _ in range(3)]
    lbs_pred = garment_around_body(rng, body_v, body_n, sel)
    root = rng.normal(0.0, 0.05, (nbatch, T, 3)).astype(F32)
    garment = (body_v[:, sel] + rng.normal(0.0, 0.01, (F_, Vg, 3))).astype(F32).reshape(nbatch, T, Vg, 3) - root[:, :, None, :]
    return dict(seed=seed, nbatch=nbatch, T=T, Vg=Vg, body=base["body"], template_faces=base["template_faces"], rounds=rounds,
                lbs_pred_garment_v=lbs_pred.reshape(nbatch, T, Vg, 3),
                inputs=dict(pose_torch=base["batch"]["pose_torch"], smpl_vertices_torch=base["batch"]["smpl_vertices_torch"],
                            smpl_root_joints_torch=root, garment_torch=garment.astype(F32)))


def stage2_loss_checksum(case):
    items = list(case["rounds"]) + [case["lbs_pred_garment_v"]] + [v for _, v in sorted(case["inputs"].items())]
    return np.array([float(np.asarray(a, dtype=np.float64).sum()) for a in items])


def stage1_loss_case(seed=210, N=256, C=7, P=64, pad_batch=4):
    """The inputs of tests/golden/stage1_loss.npz (written by tests/golden/make_golden_stage1_loss.py, which runs the reference's own
    `temporal_loss_PCA` on them): the T-pose body and the 64-vertex quad-cylinder template of refine_golden_case with its quads split into
    triangles (`garment_f_3`), logits of a few units for nbatch * T * N points with labels over all C classes, P PCA coefficients and targets,
    a `tpose_garment` placed around the T-pose body (garment_around_body; garment vertex i follows body vertex sel[i]) minus the root joint,
    `garment_template_vertices` = tpose_garment + N(0, 0.01), and args.batch_size = pad_batch > nbatch, so that the Laplacian term's padding
    with copies of item 0 is exercised.  stage1_loss_checksum() guards against generator drift."""
    base = refine_golden_case()
    nbatch, T, Vg = base["nbatch"], base["T"], base["Vg"]
    rng = np.random.default_rng(seed)
    body_v = base["batch"]["Tpose_smpl_vertices_torch"].reshape(nbatch, -1, 3)
    root = base["batch"]["Tpose_smpl_root_joints_torch"].reshape(nbatch, 1, 3)
    body_n = vertex_normals(body_v, base["body"]["faces"])
    sel = rng.permutation(body_v.shape[1])[:Vg]
    tpose_garment = (garment_around_body(rng, body_v, body_n, sel) - root).astype(F32)
    template = (tpose_garment + rng.normal(0.0, 0.01, (nbatch, Vg, 3))).astype(F32)
    quads = base["template_faces"]
    faces3 = np.concatenate([[q[[0, 1, 2]], q[[0, 2, 3]]] for q in quads], 0).astype(np.int32)      # mesh_utils.quads2tris
    logits = (rng.standard_normal((nbatch * T, N, C)) * 2.0).astype(F32)
    labels = rng.integers(0, C, (nbatch, T, N)).astype(np.int64)
    coeff = rng.standard_normal((nbatch, P)).astype(F32)
    coeff_gt = (coeff + rng.normal(0.0, 0.3, (nbatch, P))).astype(F32)
    return dict(seed=seed, nbatch=nbatch, T=T, N=N, C=C, P=P, Vg=Vg, pad_batch=pad_batch, body=base["body"],
                output=dict(sem_logits=logits, garment_PCA_coeff=coeff, tpose_garment=tpose_garment, garment_f_3=faces3),
                inputs=dict(pose_torch=base["batch"]["pose_torch"], pcd_label_torch=labels, PCACoeff=coeff_gt, garment_template_vertices=template,
                            Tpose_smpl_vertices_torch=base["batch"]["Tpose_smpl_vertices_torch"],
                            Tpose_smpl_root_joints_torch=base["batch"]["Tpose_smpl_root_joints_torch"]))


def stage1_loss_checksum(case):
    items = [v for _, v in sorted(case["output"].items())] + [v for _, v in sorted(case["inputs"].items())]
    return np.array([float(np.asarray(a, dtype=np.float64).sum()) for a in items])


def mgn_displacement_state_dict(vg, seed=0):
    """Seeded weights under the reference's names for the MGN variant's `displacement_encoder` (modules/mesh_encoder.py:518-524:
    Linear 512 -> 1024 -> 2048 -> 3 vg), drawn like torch's default Linear initialisation (uniform +-1/sqrt(in)).  numpy, fp32."""
    rng = np.random.default_rng(seed)
    sd = {}
    for i, (cin, cout) in zip((0, 2, 4), ((512, 1024), (1024, 2048), (2048, vg * 3))):
        b = 1.0 / np.sqrt(cin)
        sd["displacement_encoder.%d.weight" % i] = ((rng.random((cout, cin)) * 2 - 1) * b).astype(F32)
        sd["displacement_encoder.%d.bias" % i] = ((rng.random(cout) * 2 - 1) * b).astype(F32)
    return sd


def mgn_golden_case(seed=90, nbatch=2, T=3):
    """The inputs of tests/golden/mgn.npz (written by tests/golden/make_golden_mgn.py, which runs the reference's own MGN variant on them):
    a 320-vertex body cylinder, a 160-vertex quad-cylinder garment template, per-FRAME skinning weights and joint regressors (the clip's
    tables with a per-frame perturbation of their non-zero entries, renormalised), per-clip PCA garments, per-frame garment summaries
    and per-frame displaced garments for lbs_garment_MGN."""
    sc = garment_scene(nbatch, T, 4, body_rc=(16, 20), garment_rc=(10, 16), seed=seed)
    rng = np.random.default_rng(seed + 11)
    gv, gq = sc["template"]
    Vg = gv.shape[0]
    batch = dict(sc["batch"])
    for key, axis in (("T_lbs_weights", -1), ("T_J_regressor", -1)):
        t = batch[key] * (1 + 0.2 * rng.random(batch[key].shape)).astype(F32)
        batch[key] = (t / t.sum(axis, keepdims=True)).astype(F32)
    tpose_garment = (gv[None] + rng.standard_normal((nbatch, Vg, 3)) * 0.004).astype(F32)
    garment_summary = (rng.random((nbatch, T, 512)) * rng.random((nbatch, T, 512))).astype(F32)
    pred_template = (tpose_garment[:, None] + rng.standard_normal((nbatch, T, Vg, 3)) * 0.01).astype(F32)
    return dict(seed=seed, nbatch=nbatch, T=T, Vg=Vg, batch=batch, body=sc["body"], template_verts=gv, template_faces=gq,
                tpose_garment=tpose_garment, garment_summary=garment_summary, pred_template=pred_template)


def mgn_grad_targets(case, posed, seed=190, body_scale=(1.5, 1.0, 1.5)):
    """The loss inputs of tests/golden/mgn_grad.npz (written by tests/golden/make_golden_mgn_grad.py, which runs the reference's MGN forward,
    its `temporal_loss_PCA_LBS` and autograd on mgn_golden_case plus these): random root joints, a `garment_torch` within about a centimetre of
    `posed` (nbatch, T, Vg, 3) -- the reference's own forward output for the case, tests/golden/mgn.npz `fwd_posed` -- relative to the root, as
    the loss adds it back, and the loss's body `smpl_vertices_torch` = the scene's, widened by body_scale about each frame's centroid: against
    the scene's own body 81.9 % of the posed garment penetrates, against the widened one 53.6 % (the generator asserts 20-80 %), with no
    vertex closer than 1e-4 to the tangent plane of its nearest body vertex.  mgn_grad_checksum() guards against generator drift."""
    nbatch, T, Vg = case["nbatch"], case["T"], case["Vg"]
    rng = np.random.default_rng(seed)
    root = rng.normal(0.0, 0.05, (nbatch, T, 3)).astype(F32)
    garment = (np.asarray(posed, F32).reshape(nbatch, T, Vg, 3) + rng.normal(0.0, 0.01, (nbatch, T, Vg, 3))).astype(F32) - root[:, :, None, :]
    body = case["batch"]["smpl_vertices_torch"]
    centre = body.mean(2, keepdims=True)
    body = ((body - centre) * np.asarray(body_scale, F32) + centre).astype(F32)
    return dict(garment_torch=garment.astype(F32), smpl_root_joints_torch=root, smpl_vertices_torch=body)


def mgn_grad_checksum(case, targets):
    items = [case["tpose_garment"], case["garment_summary"]] + [v for _, v in sorted(case["batch"].items())] + [v for _, v in sorted(targets.items())]
    items += [v for _, v in sorted(mgn_displacement_state_dict(case["Vg"], seed=case["seed"] + 100).items())]
    return np.array([float(np.asarray(a, dtype=np.float64).sum()) for a in items])


def encoder_state_dict(shapes, seed=0):
    """Seeded weights for a PointNet++ encoder / PCAGarmentEncoderSeg given its state-dict {key: shape} (keys drawn in sorted order, so
    the reference's model and this package's give the same values).  Multi-dimensional weights: kaiming-normal over the fan-in.  Every
    BatchNorm (a prefix with a `running_mean`): scale +-U[0.5,1.5] (random sign), shift N(0,0.1), running mean N(0,0.2), running
    variance U[0.5,1.5] -- including the plain nn.BatchNorm1d layers of the PCA head, which encoder.seed_encoder leaves at N(0,0.1) and
    so almost switches off.  Other vectors (conv biases): N(0,0.1).  numpy; num_batches_tracked = 0 (int64), everything else fp32."""
    rng = np.random.default_rng(seed)
    bn = {k[:-len("running_mean")] for k in shapes if k.endswith("running_mean")}
    sd = {}
    for k in sorted(shapes):
        shape = tuple(int(s) for s in shapes[k])
        prefix, leaf = k[:k.rfind(".") + 1], k[k.rfind(".") + 1:]
        if leaf == "num_batches_tracked":
            sd[k] = np.zeros(shape, np.int64)
        elif prefix in bn:
            if leaf == "weight":
                v = (rng.random(shape) + 0.5) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
            elif leaf == "running_var":
                v = rng.random(shape) + 0.5
            else:
                v = rng.standard_normal(shape) * (0.2 if leaf == "running_mean" else 0.1)
            sd[k] = v.astype(F32)
        elif len(shape) > 1:
            sd[k] = (rng.standard_normal(shape) * np.sqrt(2.0 / np.prod(shape[1:]))).astype(F32)
        else:
            sd[k] = (rng.standard_normal(shape) * 0.1).astype(F32)
    return sd


def state_dict_checksum(sd):
    """Per-key float64 sums in sorted key order: detects drift of a seeded state dict between a generator and its tests."""
    return np.array([float(np.asarray(sd[k], dtype=np.float64).sum()) for k in sorted(sd)])


def encoder_golden_case(seed=120):
    """The inputs of tests/golden/encoder.npz (written by tests/golden/make_golden_encoder.py, which runs the reference's own
    PCAGarmentEncoderSeg and Pointnet2MSGSEG on them).
    E1: two clips of two N = 6890 frames whose geometries give the garment class very different logit ranges under the seeded weights:
    frame 0 = 70 % points on a line interleaved with 30 % isolated far points, frame 1 = the unit cube, frame 2 = a 0.01-wide cube,
    frame 3 = a 0.3-wide cube; the PCA basis (72 random components, a non-zero mean, a per-coordinate scale) and a 16 x 16 quad
    cylinder template.  E2/E3: a (2, 2048, 6) cloud (xyz in the unit cube + three N(0,1) feature channels)."""
    rng = np.random.default_rng(seed)
    N = 6890
    line = unit_cloud(1, N, seed=seed + 1)[0] * np.array([3, 0, 0], F32)
    far = unit_cloud(1, N, seed=seed + 2)[0] * F32(20) + F32(100)
    f0 = np.where((rng.random(N) < 0.7)[:, None], line, far)
    frames = [f0, unit_cloud(1, N, seed=seed + 3)[0], unit_cloud(1, N, seed=seed + 4)[0] * F32(0.01),
              unit_cloud(1, N, seed=seed + 5)[0] * F32(0.3)]
    x = np.stack(frames).astype(F32).reshape(2, 2, N, 3)
    gv, gq = quad_cylinder(16, 16)
    gv = (gv * np.array([1.0, 0.45, 0.7], dtype=F32) + np.array([0, -0.2, 0], dtype=F32)).astype(F32)
    pca = dict(components=(rng.standard_normal((72, gv.size)) * 0.01).astype(F32),
               mean=(gv.reshape(-1) + rng.standard_normal(gv.size) * 0.01).astype(F32),
               explained=rng.random(72), ss_scale=(0.5 + rng.random(gv.size)).astype(np.float64))
    pc = np.concatenate([unit_cloud(2, 2048, seed=seed + 6), rng.standard_normal((2, 2048, 3)).astype(F32)], -1).astype(F32)
    return dict(seed=seed, nbatch=2, T=2, N=N, x=x, pca=pca, template=(gv, gq), pc=pc)


def encoder_golden_checksum(case):
    items = [case["x"], case["pc"], case["template"][0], case["template"][1]] + [case["pca"][k] for k in sorted(case["pca"])]
    return np.array([float(np.asarray(a, dtype=np.float64).sum()) for a in items])
