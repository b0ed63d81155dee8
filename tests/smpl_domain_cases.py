"""Poses over the whole domain of rodrigues() for the SMPL tests (test infrastructure; the package never imports it): a deterministic builder of
frames by KIND of pose -- today's N(0, 0.2^2), exact zeros, 1e-6 and 1e-3 rad where 1 - cos cancels, single-axis rotations, angles near pi, at
float32(pi), between pi and 2 pi, near 2 pi, tens of radians, and tiny and large joints mixed in one frame --, the shapes that reach the domain
edges of the fast lbs() routes and of the adjoint, the float64 rigid chain on given rotations and rest joints, and the comparison the GPU tests
use: per kind, the kernel's error against float64 must stay within 3 x max(what the fp32 restatements lose on that kind, what they lose on the
baseline kind), both measured on the same inputs."""
import numpy as np

import smpl_grad_twin as ST
from garment4d_amd import synthetic as syn

F32, F64 = np.float32, np.float64
KINDS = ("baseline", "zeros", "tiny", "small", "single_axis", "near_pi", "at_pi", "pi_to_2pi", "near_2pi", "large", "mixed")
FRAMES_PER_KIND = 3
#          V    J   NB
SHAPES = [(97,  24, 10),    # SMPL's own counts, V off every tile
          (65,  25, 8),     # NB + 9 (J - 1) = 224 exactly: the last full K slice, the js = 8 operand layout
          (65,  25, 9),     # 225: outside the fast routes and the adjoint (forward only, through the three-launch route)
          (33,  2,  1),     # the smallest chain
          (130, 5,  16)]    # a weight row that is not 16-byte aligned, NB > 10
MAX_COEFFS = 224            # g4d_lbs_one_supported, g4d_lbs_mfma_supported, g4d_smpl_grad_supported: NB + 9 (J - 1) <= 224
FACTOR = 3.0                # tests/test_smpl_grad_gpu.py's: 3 x the error fp32 makes on the same inputs
SINGLE_AXIS_VALUES = (np.pi / 2, -np.pi / 2, 0.3, -0.3, np.pi)


def in_fast_domain(J, NB):
    return NB + 9 * (J - 1) <= MAX_COEFFS


def mixed_joint(J):
    return min(3, J - 1)


def _axes(rng, J):
    a = rng.standard_normal((J, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _frame(kind, rng, J):
    """(J,3) float64 axis-angle of one frame of `kind`."""
    if kind == "baseline":
        return rng.standard_normal((J, 3)) * 0.2
    if kind == "zeros":
        return np.zeros((J, 3))
    if kind == "tiny":
        return rng.standard_normal((J, 3)) * 1e-6
    if kind == "small":
        return rng.standard_normal((J, 3)) * 1e-3
    if kind == "single_axis":
        p = np.zeros((J, 3))
        p[np.arange(J), rng.integers(0, 3, J)] = np.asarray(SINGLE_AXIS_VALUES)[rng.integers(0, len(SINGLE_AXIS_VALUES), J)]
        return p
    if kind == "near_pi":
        return _axes(rng, J) * (np.pi - 1e-3)
    if kind == "at_pi":
        return _axes(rng, J) * F64(F32(np.pi))
    if kind == "pi_to_2pi":
        return _axes(rng, J) * rng.uniform(np.pi, 2 * np.pi, (J, 1))
    if kind == "near_2pi":
        return _axes(rng, J) * (2 * np.pi + 1e-3 * rng.choice([-1.0, 1.0], (J, 1)))
    if kind == "large":
        return _axes(rng, J) * rng.uniform(10.0, 100.0, (J, 1))
    if kind == "mixed":
        p = rng.standard_normal((J, 3)) * 1e-5
        p[0] = _axes(rng, 1)[0] * (np.pi - 1e-2)
        p[mixed_joint(J)] = (0.0, 0.0, 1.5)
        return p
    raise ValueError(kind)


def case(V, J, NB, seed):
    """-> (P, betas (B,NB) f32, pose (B,J*3) f32, kinds: one label per frame); B = 3 frames per kind = 33: no multiple of the 8-frame group of the
    one-launch kernel, of the 16-frame MFMA tile or of the adjoint's 2 frames per workgroup.  betas: N(0,1) scaled per frame from 0.5 to 3."""
    P = syn.smpl_like_params(V=V, J=J, num_betas=NB, seed=seed)
    rng = np.random.default_rng(seed + 1)
    kinds = [k for k in KINDS for _ in range(FRAMES_PER_KIND)]
    B = len(kinds)
    pose = np.stack([_frame(k, rng, J) for k in kinds]).reshape(B, J * 3).astype(F32)
    betas = (rng.standard_normal((B, NB)) * np.linspace(0.5, 3.0, B)[:, None]).astype(F32)
    return P, betas, pose, kinds


def one_frame_per_kind(betas, pose, kinds):
    idx = [kinds.index(k) for k in KINDS]
    return np.ascontiguousarray(betas[idx]), np.ascontiguousarray(pose[idx]), list(KINDS)


def angles(pose, J):
    """(B,J) rotation angles |theta| in float64 of a float32 pose."""
    return np.linalg.norm(np.asarray(pose, F64).reshape(len(pose), J, 3), axis=2)


def checksum(betas, pose):
    """Order-sensitive sums of the two arrays in float64 (exact up to the last bits of the float64 sum: compared with rtol 1e-12)."""
    b, p = betas.astype(F64).ravel(), pose.astype(F64).ravel()
    return np.array([(b * np.cos(np.arange(b.size))).sum(), (p * np.cos(np.arange(p.size))).sum(), np.abs(p).sum()])


def upstream(B, V, J, which, seed):
    """(d_verts, d_joints) ~ N(0,1) in float32, None where `which` ('v', 'j', 'both') leaves one out."""
    rng = np.random.default_rng(seed)
    gv, gj = rng.standard_normal((B, V, 3)).astype(F32), rng.standard_normal((B, J, 3)).astype(F32)
    return (gv if which in ("v", "both") else None), (gj if which in ("j", "both") else None)


def rigid_f64(R, Jr, parents):
    """batch_rigid_transform in float64 on given rotations (B,J,3,3) and rest joints (B,J,3), as tests/smpl_grad_twin.py: forward chains them:
    -> GR (B,J,3,3), Gt (B,J,3) (the posed joints), At (B,J,3) (A = [GR | At])."""
    R, Jr = np.asarray(R, F64), np.asarray(Jr, F64)
    GR, Gt = np.zeros_like(R), np.zeros_like(Jr)
    GR[:, 0], Gt[:, 0] = R[:, 0], Jr[:, 0]
    for j in range(1, R.shape[1]):
        p = int(parents[j])
        GR[:, j] = GR[:, p] @ R[:, j]
        Gt[:, j] = np.einsum("brc,bc->br", GR[:, p], Jr[:, j] - Jr[:, p]) + Gt[:, p]
    return GR, Gt, Gt - np.einsum("bjrc,bjc->bjr", GR, Jr)


# ------------------------------------------------------------------------------------------------------------------------- the comparison
def kind_errors(got, want, kinds):
    """{kind: max |got - want| over the frames of that kind}; got, want: (B, ...) with one frame per entry of `kinds`."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape and got.shape[0] == len(kinds), (got.shape, want.shape, len(kinds))
    err = np.abs(got - want).reshape(len(kinds), -1).max(1) if got[0].size else np.zeros(len(kinds))
    err = np.where(np.isfinite(err), err, np.inf)            # a NaN anywhere counts as an infinite error
    return {k: float(max(e for e, kk in zip(err, kinds) if kk == k)) for k in dict.fromkeys(kinds)}


def kind_bounds(refs, want, kinds, extra=0.0):
    """{kind: 3 max(e_kind, e_baseline) + extra}, e_kind = the largest error of any of the fp32 restatements `refs` against `want` on that kind."""
    e = {k: 0.0 for k in dict.fromkeys(kinds)}
    for r in refs:
        for k, v in kind_errors(r, want, kinds).items():
            e[k] = max(e[k], v)
    assert "baseline" in e and 0.0 < e["baseline"] < np.inf, e
    return {k: FACTOR * max(v, e["baseline"]) + extra for k, v in e.items()}


def parity(label, got, want, refs, kinds, extra=0.0, allow=1.0):
    """Prints one [parity] line (the worst kind's err, bound and err / bound) and returns the kinds out of bound as [(label, kind, err, bound)].
    allow: a measured and explained excess, as a multiple of the bound (the caller says where it comes from)."""
    err = kind_errors(got, want, kinds)
    bound = {k: allow * b for k, b in kind_bounds(refs, want, kinds, extra).items()}
    worst = max(err, key=lambda k: err[k] / bound[k])
    print(f"[parity] {label}: worst kind {worst}  err {err[worst]:.3e}  bound {bound[worst]:.3e}  err/bound {err[worst] / bound[worst]:.3f}"
          f"  (baseline bound {bound['baseline']:.3e}, max |want| {np.abs(want).max():.3e})")
    return [(label, k, err[k], bound[k]) for k in err if not err[k] <= bound[k]]


def parity_whole(label, got, want, refs):
    """The same for a tensor that has no frame axis (d_betas of one broadcast row): one error, bound = 3 x the restatements' error on it."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want).max()
    err = float(err) if np.isfinite(err) else np.inf
    bound = FACTOR * max(float(np.abs(np.asarray(r, F64) - want).max()) for r in refs)
    assert 0.0 < bound < np.inf
    print(f"[parity] {label}: err {err:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}  (max |want| {np.abs(want).max():.3e})")
    return [] if err <= bound else [(label, "all", err, bound)]


# ------------------------------------------------------------------------------------------------------------------------- references
def rot_input(pose, J):
    """The float64 twin's rotation matrices of an axis-angle pose, rounded to float32: the input of the pose2rot = False calls."""
    return ST.rodrigues(np.asarray(pose, F64).reshape(-1, 3))[0].reshape(len(pose), J, 3, 3).astype(F32)


def forward_refs(P, betas, pose_in, pose2rot):
    """((verts, joints) of the float64 twin, [(verts, joints) of each fp32 restatement]) on the same float32 inputs."""
    import torch
    from oracle import lbs_oracle
    want = ST.forward(betas, pose_in, P, pose2rot)
    tp = ST.torch_params(P, torch.float32)
    with torch.no_grad():
        tv, tj = ST.torch_lbs(torch.from_numpy(np.ascontiguousarray(betas)), torch.from_numpy(np.ascontiguousarray(pose_in)), tp, pose2rot)
    ov, oj = lbs_oracle.lbs(betas, pose_in, P["v_template"], P["shapedirs"], P["posedirs"], P["J_regressor"], P["parents"], P["lbs_weights"], pose2rot=pose2rot)
    return want, [(tv.numpy(), tj.numpy()), (ov, oj)]
