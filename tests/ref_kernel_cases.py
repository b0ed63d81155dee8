"""Cases and runners shared by tests/test_ref_kernels_gpu.py, tests/test_ref_kernels_cpu.py and scripts/dump_ref_kernels.py.

Three modules carry the reference extension's nine entry points (pointnet2_api.cpp): the reference build (oracle/ref_pointnet2.py,
the reference's own kernel files compiled uncontracted for gfx950), the CPU oracle (oracle.pointnet2_oracle.as_pointnet2_cuda_module())
and the product (garment4d_amd.pointnet2_cuda).  The runners below drive any of them the way the reference's Python does
(pointnet2_utils.py: temp filled with 1e10, ball idx zero-filled, gradients zero-filled) and return numpy arrays.

A case is a dict of generator arguments (json-able: kind, seed, sizes); `*_inputs(case)` rebuilds its arrays, so the recorded
fixture tests/golden/ops_ref_hip_off.npz holds arguments and outputs, never clouds.
"""
import json

import numpy as np

from garment4d_amd import synthetic as syn

FPS_SIZES = (1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64, 65, 100, 255, 256, 257, 700, 1023, 1024, 1025, 2047, 2048, 2049, 6890, 8192, 8193)
# ^ sizes at and around each power of two; 8, 9, 16, 17 are there because no other size below 33 gives the 8- and 16-thread templates
FPS_B, FPS_M_MAX = 2, 300
FIXTURE_MAX_N = 1025        # the recorded fixture keeps the cases up to this cloud size
FIXTURE_NN_ROWS = 128       # ... and of a three_nn case the first rows only
BLOCK_SIZE_MAX_N = 40000    # opt_n_threads() is compared for every n in 1..this


def cloud(kind, B, N, seed):
    """`unit`: U[0,1)^3.  `body`: shell with 30 % exact duplicates and a 15 % zero-padded tail -- ties everywhere."""
    if kind == "unit":
        return syn.unit_cloud(B, N, seed=seed)
    assert kind == "body", kind
    return syn.body_like_cloud(B, N, seed=seed, dup_frac=0.3, zero_frac=0.15)


def bits(a):
    """The bit pattern of a float32 array (int arrays pass through): what `bit for bit` compares."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def first_diff(a, b):
    d = np.argwhere(bits(a) != bits(b))
    return f"{len(d)} of {np.asarray(a).size} differ, first at {d[:3].tolist()}: {[(np.asarray(a)[tuple(i)], np.asarray(b)[tuple(i)]) for i in d[:3]]}"


def case_id(case):
    return "-".join(f"{v}" for v in case.values())


# ---------------------------------------------------------------------------------------------------------------- FPS
def fps_cases():
    out = [dict(op="fps", kind=kind, n=n, seed=1000 + n, special="") for n in FPS_SIZES for kind in ("unit", "body")]
    # a NaN point (never closer than anything: its min-distance stays at the caller's 1e10) and an inf coordinate
    out += [dict(op="fps", kind="unit", n=700, seed=77, special="nan_point"), dict(op="fps", kind="body", n=257, seed=78, special="nan_point"),
            dict(op="fps", kind="unit", n=700, seed=79, special="inf_coord"), dict(op="fps", kind="body", n=257, seed=80, special="inf_coord")]
    return out


def fps_inputs(case):
    n = case["n"]
    xyz = cloud(case["kind"], FPS_B, n, case["seed"])
    if case["special"] == "nan_point":
        xyz[0, n // 3] = np.nan
        xyz[1, 1, 2] = np.nan
    elif case["special"] == "inf_coord":
        xyz[0, n // 3, 1] = np.inf
        xyz[1, 5, 0] = -np.inf
    return xyz, min(n, FPS_M_MAX)


def run_fps(mod, device, xyz, m):
    import torch
    B, N, _ = xyz.shape
    x = torch.from_numpy(xyz).to(device)
    temp = torch.full((B, N), 1e10, dtype=torch.float32, device=device)          # pointnet2_utils.py:26
    idx = torch.full((B, m), -1, dtype=torch.int32, device=device)
    mod.furthest_point_sampling_wrapper(B, N, m, x, temp, idx)
    return idx.cpu().numpy(), temp.cpu().numpy()


# --------------------------------------------------------------------------------------------------------- ball query
_BQ_EXTRA = [  # (B, N, M, radius, nsample, kind): nsample 1 / 5 / 64 / 128, radius 0, N and M off the 256-thread block
    (2, 333, 40, 0.3, 1, "body"), (2, 333, 40, 0.0, 5, "body"), (2, 1025, 77, 0.25, 64, "body"), (1, 700, 33, 1.5, 128, "body"),
    (2, 257, 257, 0.1, 5, "unit"), (2, 8192, 300, 0.0, 16, "unit"),
]


def ball_cases():
    from test_ops_gpu import BQ_CASES
    out = [dict(op="ball", B=B, n=N, m=M, radius=r, nsample=ns, kind="body" if N % 2 else "unit", seed=N + ns)
           for B, N, M, r, ns in BQ_CASES if N <= 8192]
    out += [dict(op="ball", B=B, n=N, m=M, radius=r, nsample=ns, kind=kind, seed=N + ns) for B, N, M, r, ns, kind in _BQ_EXTRA]
    return out


def ball_inputs(case):
    """The cloud and M queries sitting exactly on points of it; query 0 has no neighbour at all, query 1 (body clouds) sits on a
    point the cloud holds more than once (the lower index must come first), query 2 (body clouds) on the zero padding."""
    B, N, M = case["B"], case["n"], case["m"]
    xyz = cloud(case["kind"], B, N, case["seed"])
    q = xyz[:, np.random.default_rng(M).permutation(N)[:M]].copy()
    q[:, 0] = 7.0
    if case["kind"] == "body" and M > 2:
        nd, nz = int(N * 0.3), int(N * 0.15)
        q[:, 1] = xyz[:, N - nd - nz]
        assert all(int((xyz[b] == q[b, 1]).all(-1).sum()) >= 2 for b in range(B)), "query 1 must sit on a duplicated point"
        q[:, 2] = xyz[:, N - 1]
        assert not q[:, 2].any()
    return xyz, np.ascontiguousarray(q)


def run_ball(mod, device, xyz, q, radius, nsample):
    import torch
    B, N, _ = xyz.shape
    M = q.shape[1]
    idx = torch.zeros((B, M, nsample), dtype=torch.int32, device=device)          # pointnet2_utils.py:218
    mod.ball_query_wrapper(B, N, M, radius, nsample, torch.from_numpy(q).to(device), torch.from_numpy(xyz).to(device), idx)
    return idx.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------- three_nn
def nn_cases():
    from test_ops_gpu import _nn_cases
    return [dict(op="nn", name=name) for name in _nn_cases()] + [dict(op="nn", name=f"tie_heavy_known_{m}") for m in (1, 2, 3)]


def nn_inputs(case):
    from test_ops_gpu import _nn_cases
    name = case["name"]
    if name.startswith("tie_heavy_known_"):          # m = 1, 2, 3 out of a tie-heavy cloud: the sentinels (1e40 -> inf, index 0) show for m < 3
        m = int(name.rsplit("_", 1)[1])
        return syn.unit_cloud(2, 300, seed=40 + m), np.ascontiguousarray(cloud("body", 2, 8, 50 + m)[:, 8 - m - 1:8 - 1])
    un, kn = _nn_cases()[name]
    return np.ascontiguousarray(un, dtype=np.float32), np.ascontiguousarray(kn, dtype=np.float32)


def run_nn(mod, device, unknown, known):
    import torch
    B, n, _ = unknown.shape
    m = known.shape[1]
    dist2 = torch.full((B, n, 3), -7.0, dtype=torch.float32, device=device)
    idx = torch.full((B, n, 3), -7, dtype=torch.int32, device=device)
    mod.three_nn_wrapper(B, n, m, torch.from_numpy(unknown).to(device), torch.from_numpy(known).to(device), dist2, idx)
    return dist2.cpu().numpy(), idx.cpu().numpy()


# ------------------------------------------------------------------------------------- group / gather / interpolate
GGI_SHAPES = [(2, 3, 1024, 256, 32), (2, 99, 1024, 256, 16), (1, 195, 256, 64, 64), (2, 7, 100, 13, 5)]   # test_group_gather_interp_vs_oracle


def ggi_inputs(B, C, N, P, S):
    rng = np.random.default_rng(C + N)
    pts = rng.standard_normal((B, C, N)).astype(np.float32)
    idx = rng.integers(0, N, size=(B, P, S)).astype(np.int32)
    i3 = rng.integers(0, N, size=(B, P, 3)).astype(np.int32)
    w = rng.random((B, P, 3)).astype(np.float32)
    return pts, idx, i3, w


def run_group(mod, device, pts, idx):
    import torch
    B, C, N = pts.shape
    _, P, S = idx.shape
    out = torch.full((B, C, P, S), -7.0, dtype=torch.float32, device=device)
    mod.group_points_wrapper(B, C, N, P, S, torch.from_numpy(pts).to(device), torch.from_numpy(idx).to(device), out)
    return out.cpu().numpy()


def run_gather(mod, device, pts, idx):
    import torch
    B, C, N = pts.shape
    M = idx.shape[1]
    out = torch.full((B, C, M), -7.0, dtype=torch.float32, device=device)
    mod.gather_points_wrapper(B, C, N, M, torch.from_numpy(pts).to(device), torch.from_numpy(np.ascontiguousarray(idx)).to(device), out)
    return out.cpu().numpy()


def run_interp(mod, device, pts, i3, w):
    import torch
    B, C, M = pts.shape
    n = i3.shape[1]
    out = torch.full((B, C, n), -7.0, dtype=torch.float32, device=device)
    mod.three_interpolate_wrapper(B, C, M, n, torch.from_numpy(pts).to(device), torch.from_numpy(i3).to(device), torch.from_numpy(w).to(device), out)
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- the backwards
def exact_grad_inputs(B, C, N, P, S, collide):
    """Integer-valued cotangents (|v| <= 8) and weights in {0, 0.25, 0.5, 1}: every product is a multiple of 0.25 and every partial
    sum far below 2^24 quarter-units, so the sums are exact in any order and the atomics of the three implementations must agree
    bit for bit.  `collide`: every index of a neighbourhood (and a whole block of neighbourhoods) points at one source."""
    rng = np.random.default_rng(B + C + N + P + S)
    idx = rng.integers(0, N, size=(B, P, S)).astype(np.int32)
    i3 = rng.integers(0, N, size=(B, P, 3)).astype(np.int32)
    if collide:
        idx[:] = idx[:, :, :1]                 # a neighbourhood = S copies of one source
        idx[:, : P // 2] = N - 1               # ... and half of all neighbourhoods the same one
        i3[:] = i3[:, :, :1]
        i3[:, : P // 2] = 0
    go_group = rng.integers(-8, 9, size=(B, C, P, S)).astype(np.float32)
    go_gather = rng.integers(-8, 9, size=(B, C, P)).astype(np.float32)
    go_interp = rng.integers(-8, 9, size=(B, C, P)).astype(np.float32)
    w = rng.choice(np.array([0.0, 0.25, 0.5, 1.0], np.float32), size=(B, P, 3)).astype(np.float32)
    return idx, i3, w, go_group, go_gather, go_interp


def run_group_grad(mod, device, go, idx, N):
    import torch
    B, C, P, S = go.shape
    gp = torch.zeros((B, C, N), dtype=torch.float32, device=device)               # pointnet2_utils.py:190
    mod.group_points_grad_wrapper(B, C, N, P, S, torch.from_numpy(go).to(device), torch.from_numpy(idx).to(device), gp)
    return gp.cpu().numpy()


def run_gather_grad(mod, device, go, idx, N):
    import torch
    B, C, M = go.shape
    gp = torch.zeros((B, C, N), dtype=torch.float32, device=device)               # pointnet2_utils.py:67
    mod.gather_points_grad_wrapper(B, C, N, M, torch.from_numpy(go).to(device), torch.from_numpy(np.ascontiguousarray(idx)).to(device), gp)
    return gp.cpu().numpy()


def run_interp_grad(mod, device, go, i3, w, M):
    import torch
    B, C, n = go.shape
    gp = torch.zeros((B, C, M), dtype=torch.float32, device=device)               # pointnet2_utils.py:146
    mod.three_interpolate_grad_wrapper(B, C, n, M, torch.from_numpy(go).to(device), torch.from_numpy(i3).to(device), torch.from_numpy(w).to(device), gp)
    return gp.cpu().numpy()


# ---------------------------------------------------------------------------------------------- the recorded fixture
def fixture_cases():
    """The subset of the cases above that tests/golden/ops_ref_hip_off.npz records: clouds of at most FIXTURE_MAX_N points."""
    fps = [c for c in fps_cases() if c["n"] <= FIXTURE_MAX_N]
    ball = [c for c in ball_cases() if c["n"] <= FIXTURE_MAX_N and c["B"] * c["m"] * c["nsample"] <= 8192]
    nn = [dict(op="nn", name=n) for n in ("queries_outside_the_box", "fewer_than_three_known", "non_finite_known_and_queries", "tie_heavy_known_1", "tie_heavy_known_3")]
    return fps + ball + nn


def fixture_outputs(case, mod, device):
    """{name: array} of what the fixture keeps of `case`, computed through `mod` (the reference build when recording, the oracle when
    checking)."""
    if case["op"] == "fps":
        idx, temp = run_fps(mod, device, *fps_inputs(case))
        return {"idx": idx, "temp": temp}
    if case["op"] == "ball":
        xyz, q = ball_inputs(case)
        return {"idx": run_ball(mod, device, xyz, q, case["radius"], case["nsample"])}
    un, kn = nn_inputs(case)
    d2, idx = run_nn(mod, device, un, kn)
    return {"dist2": d2[:, :FIXTURE_NN_ROWS], "idx": idx[:, :FIXTURE_NN_ROWS]}


def case_key(case):
    return json.dumps(case, sort_keys=True)
