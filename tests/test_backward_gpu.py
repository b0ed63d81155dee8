"""The training route's backward: the three scatter-add kernels of csrc/pointnet2_ops.hip (group_grad_kernel, which also serves
g4d_gather_grad_f32, and three_interp_grad_kernel) and the gradients of whole SA / FP modules and the encoder, against float64
references (oracle/autograd_twin.py).

Kernel level, two modes:
  * exact -- integer grad_out in [-4, 4] and weights that are multiples of 1/4, every partial sum below 2^24 (asserted): every
    summation order gives the same fp32 result, so the kernel must equal the float64 scatter-add BIT FOR BIT, whatever the contention.
  * float -- random normal grad_out / weights: |got - ref64| <= (k + 2) 2^-24 sum |term| per element (k contributions).
Index sets are the ones training produces: ball-query rows padded with their first hit, zero-padded tails, isolated centroids, FPS
repeats, three_nn over duplicated known points, fewer than 3 known points -- plus channel counts around kCT = 8 and lengths around the
256-thread block.

Module level: one forward + backward of the HIP op-by-op route (train mode, batch-statistics BN) against a float64 CPU copy of the
module that replays the HIP run's FPS / ball-query / three_nn outputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from garment4d_amd import pointnet2_cuda as P2
from garment4d_amd import pointnet2_modules as PM
from garment4d_amd import pointnet2_utils as PU
from garment4d_amd import synthetic as syn
from garment4d_amd.encoder import Pointnet2MSGSEG, seed_encoder
from oracle import autograd_twin as AT

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _grad_out(rng, shape, exact):
    if exact:
        return rng.integers(-4, 5, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _weights(rng, shape, exact):
    if exact:
        return (rng.integers(0, 5, size=shape) / 4).astype(np.float32)
    return rng.random(shape).astype(np.float32)


def _check(got, ref, exact, what):
    s, k, a = ref
    if exact:
        # integer / quarter-integer terms with every partial sum below 2^24 (2^22 with quarters): no fp32 rounding in any order
        assert a.size == 0 or a.max() < 2 ** 22, f"{what}: exact-mode precondition broken (sum |term| = {a.max()})"
        assert np.array_equal(got, s.astype(np.float32)), \
            f"{what}: {int((got != s).sum())} elements differ from the exact scatter-add (max |diff| {np.abs(got - s).max()})"
    else:
        bound = AT.atomic_sum_bound(k[:, None, :], a)
        err = np.abs(got.astype(np.float64) - s)
        bad = err > bound
        assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the (k + 2) 2^-24 sum|term| bound, worst err {err.max()}"


def run_group_grad(go, idx, N, exact, what=""):
    """grouping_operation backward through autograd (the training route) against the exact scatter-add."""
    ref = AT.group_grad_exact(go, idx, N)              # asserts 0 <= idx < N before anything is launched
    B, C = go.shape[:2]
    f = torch.zeros((B, C, N), device="cuda", requires_grad=True)
    PU.grouping_operation(f, dev(idx)).backward(dev(go))
    _check(host(f.grad), ref, exact, what or f"group_grad B={B} C={C} N={N} idx{idx.shape}")


def run_gather_grad(go, idx, N, exact, what=""):
    ref = AT.gather_grad_exact(go, idx, N)
    B, C = go.shape[:2]
    f = torch.zeros((B, C, N), device="cuda", requires_grad=True)
    PU.gather_operation(f, dev(idx)).backward(dev(go))
    _check(host(f.grad), ref, exact, what or f"gather_grad B={B} C={C} N={N} idx{idx.shape}")


def run_interp_grad(go, idx, w, m, exact, what=""):
    ref = AT.three_interpolate_grad_exact(go, idx, w, m)
    B, C = go.shape[:2]
    f = torch.zeros((B, C, m), device="cuda", requires_grad=True)
    PU.three_interpolate(f, dev(idx), dev(w)).backward(dev(go))
    _check(host(f.grad), ref, exact, what or f"three_interp_grad B={B} C={C} m={m} idx{idx.shape}")


# ------------------------------------------------------------------------------------------------------------- index sets
def _fps_chain(xyz, npoints):
    """The encoder's sampled clouds [xyz, l1, l2, ...] (HIP FPS + gather, as the training route computes them)."""
    out = [dev(xyz)]
    for m in npoints:
        idx = PU.furthest_point_sample(out[-1], m)
        out.append(PU.gather_operation(out[-1].transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous())
    return out


def _ball_idx(xyz_t, new_xyz_t, r, ns):
    return host(PU.ball_query(r, ns, xyz_t, new_xyz_t))


@pytest.fixture(scope="module")
def cfg2_levels():
    """cfg2 (B = 8, N = 8192) clouds of the three SA levels on a uniform and a body-like (duplicates + zero tail) cloud."""
    return {kind: _fps_chain(cloud(8, 8192, seed=31), [1024, 256, 64])
            for kind, cloud in (("unit", syn.unit_cloud), ("body", syn.body_like_cloud))}


# (level, C of the grouped features, radius, nsample): SA-1 groups xyz only (input_channels = 0); SA-2 / SA-3 group xyz and features
SA_LEVELS = [(0, 3, 0.05, 16), (0, 3, 0.1, 32), (1, 96, 0.1, 16), (1, 3, 0.2, 32), (2, 192, 0.2, 32), (2, 131, 0.4, 64)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("kind", ["unit", "body"])
@pytest.mark.parametrize("lvl,C,r,ns", SA_LEVELS)
def test_group_grad_ball_query_indices_cfg2(cfg2_levels, kind, lvl, C, r, ns, exact):
    """The encoder's training shapes per SA level, indices from the real ball query: rows padded with their first hit (73 % of the
    SA-1 rows on uniform clouds) and, on the body-like cloud, the zero-padded tail's rows all pointing at the same few points."""
    L = cfg2_levels[kind]
    idx = _ball_idx(L[lvl], L[lvl + 1], r, ns)
    N = L[lvl].shape[1]
    go = _grad_out(np.random.default_rng(lvl * 100 + ns), (8, C) + idx.shape[1:], exact)
    run_group_grad(go, idx, N, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
def test_group_grad_cfg5(exact):
    """cfg5: B = 32, N = 32768, SA-1 (1024 centroids, nsample 32) on the xyz channels."""
    L = _fps_chain(syn.body_like_cloud(32, 32768, seed=5), [1024])
    idx = _ball_idx(L[0], L[1], 0.05, 32)
    run_group_grad(_grad_out(np.random.default_rng(5), (32, 3, 1024, 32), exact), idx, 32768, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("C", [1, 9, 131])
def test_group_grad_isolated_centroids(C, exact):
    """Every ball holds only its centre: all nsample slots repeat one index (64 same-address atomics per row, in one wave)."""
    xyz = syn.unit_cloud(2, 2048, seed=8)
    x = dev(xyz)
    idx = _ball_idx(x, dev(xyz[:, :300]), 1e-6, 64)
    assert (idx == np.arange(300)[None, :, None]).all()
    run_group_grad(_grad_out(np.random.default_rng(C), (2, C, 300, 64), exact), idx, 2048, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("C", [3, 9])
def test_group_grad_all_indices_zero(C, exact):
    """P * S = 65536 contributions per channel to ONE address: the worst contention there is."""
    idx = np.zeros((2, 1024, 64), np.int32)
    run_group_grad(_grad_out(np.random.default_rng(C), (2, C, 1024, 64), exact), idx, 100, exact)


def _padded_idx(rng, B, P, S, N):
    """Random rows, a third of them padded with their first entry, the last quarter pointing at index 0 (a zero tail)."""
    idx = rng.integers(0, N, size=(B, P, S)).astype(np.int32)
    pad = rng.random((B, P)) < 0.33
    cut = rng.integers(1, S + 1, size=(B, P))
    fill = np.arange(S)[None, None, :] >= cut[..., None]
    idx = np.where(pad[..., None] & fill, idx[..., :1], idx)
    idx[:, P - P // 4:] = 0
    return np.ascontiguousarray(idx, dtype=np.int32)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("P,S", [(1, 1), (255, 1), (257, 1), (1, 257), (5, 51), (37, 27)])
@pytest.mark.parametrize("C", [1, 3, 7, 8, 9, 131, 259])
def test_group_grad_channel_and_length_edges(C, P, S, exact):
    """C around kCT = 8 (partial channel chunks) and e_total = P * S of 1, 255, 257, 999 (partial 256-thread blocks)."""
    rng = np.random.default_rng(C * 1000 + P * S)
    idx = _padded_idx(rng, 2, P, S, 300)
    run_group_grad(_grad_out(rng, (2, C, P, S), exact), idx, 300, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("C", [3, 9])
def test_gather_grad_fps_with_repeats(C, exact):
    """FPS on a cloud with 10 distinct points sampled to 48: the indices repeat."""
    rng = np.random.default_rng(12)
    base = rng.random((2, 10, 3)).astype(np.float32)
    xyz = np.ascontiguousarray(base[:, rng.integers(0, 10, size=64)])
    idx = host(PU.furthest_point_sample(dev(xyz), 48))
    assert all(len(np.unique(idx[b])) < 48 for b in range(2))
    run_gather_grad(_grad_out(rng, (2, C, 48), exact), idx, 64, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("lvl", [0, 1, 2])
def test_gather_grad_cfg2_fps(cfg2_levels, lvl, exact):
    """new_xyz = gather(xyz, fps idx) at the encoder's three levels (the route of the xyz gradient through the centroids)."""
    src = cfg2_levels["body"][lvl]
    m = (1024, 256, 64)[lvl]
    idx = host(PU.furthest_point_sample(src, m))
    run_gather_grad(_grad_out(np.random.default_rng(lvl), (8, 3, m), exact), idx, src.shape[1], exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("M", [1, 255, 257])
@pytest.mark.parametrize("C", [1, 7, 8, 9, 259])
def test_gather_grad_channel_and_length_edges(C, M, exact):
    rng = np.random.default_rng(C * 7 + M)
    idx = rng.integers(0, 40, size=(2, M)).astype(np.int32)
    run_gather_grad(_grad_out(rng, (2, C, M), exact), idx, 40, exact)


def _module_weights(dist):
    """PointnetFPModule's interpolation weights from three_nn distances (inf distance -> weight 0)."""
    d = torch.from_numpy(dist)
    r = 1.0 / (d + 1e-8)
    return (r / r.sum(dim=2, keepdim=True)).numpy().astype(np.float32)


def _nn_case(unknown, known, exact, rng):
    d, i = PU.three_nn(dev(unknown), dev(known))
    d, i = host(d), host(i)
    if exact:
        w = _weights(rng, i.shape, True)
        w[np.isinf(d)] = 0.0                          # the slots three_nn could not fill carry weight 0, as the module's weights do
    else:
        w = _module_weights(d)
    return i, w, d


# (n, m, C) of the encoder's FP levels at cfg2
FP_LEVELS = [(256, 64, 384), (1024, 256, 256), (8192, 1024, 128)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("kind", ["unit", "body"])
@pytest.mark.parametrize("n,m,C", FP_LEVELS)
def test_three_interp_grad_fp_levels_cfg2(cfg2_levels, kind, n, m, C, exact):
    L = cfg2_levels[kind]
    lvl = {8192: 0, 1024: 1, 256: 2}[n]
    rng = np.random.default_rng(n + C)
    i, w, _ = _nn_case(host(L[lvl]), host(L[lvl + 1]), exact, rng)
    run_interp_grad(_grad_out(rng, (8, C, n), exact), i, w, m, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
def test_three_interp_grad_duplicated_known_points(exact):
    """Known points with exact duplicates and a zero tail (body-like): tied neighbours, many unknowns sharing the same three."""
    rng = np.random.default_rng(21)
    known = syn.body_like_cloud(2, 700, seed=21, dup_frac=0.5, zero_frac=0.2)
    unknown = syn.body_like_cloud(2, 5000, seed=22)
    i, w, _ = _nn_case(unknown, known, exact, rng)
    run_interp_grad(_grad_out(rng, (2, 9, 5000), exact), i, w, 700, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("m", [1, 2])
def test_three_interp_grad_fewer_than_three_known(m, exact):
    """m < 3: the slots three_nn leaves unfilled get weight 0 and must contribute nothing."""
    rng = np.random.default_rng(m)
    i, w, d = _nn_case(syn.unit_cloud(2, 300, seed=m), syn.unit_cloud(2, m, seed=m + 9), exact, rng)
    assert np.isinf(d[..., m:]).all() and (w[..., m:] == 0).all()
    run_interp_grad(_grad_out(rng, (2, 7, 300), exact), i, w, m, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
@pytest.mark.parametrize("C", [1, 3, 7, 8, 9, 131, 259])
def test_three_interp_grad_channel_and_length_edges(C, n, exact):
    rng = np.random.default_rng(C * 31 + n)
    m = 50
    i = rng.integers(0, m, size=(2, n, 3)).astype(np.int32)
    i[:, : n // 3] = i[:, : n // 3, :1]               # three equal neighbours (duplicated known point)
    i[:, n - n // 4:] = 0                             # a zero tail
    run_interp_grad(_grad_out(rng, (2, C, n), exact), i, _weights(rng, (2, n, 3), exact), m, exact)


# ------------------------------------------------------------------------------------------------------ offsets beyond 2^31
def test_group_grad_offsets_beyond_2_31():
    """B * C * P * S = 130 * 65536 * 256 > 2^31 (8.7 GB of grad_out): with grad_out[b, c, ...] = c + 1 the gradient is
    (c + 1) * count[k] exactly; an int32 offset would wrap for channels from 128 on."""
    B, C, N, P, S = 1, 130, 4096, 65536, 256
    assert B * C * P * S > 2 ** 31
    idx = np.random.default_rng(0).integers(0, N, size=(B, P, S)).astype(np.int32)
    idx[0, :64, :] = 0                                # a hot spot
    count = np.bincount(idx.ravel(), minlength=N).astype(np.float64)
    want = (np.arange(1, C + 1, dtype=np.float64)[:, None] * count[None, :]).astype(np.float32)
    assert want.max() < 2 ** 24
    go = torch.arange(1, C + 1, dtype=torch.float32, device="cuda").view(1, C, 1, 1).expand(B, C, P, S).contiguous()
    gp = torch.zeros((B, C, N), dtype=torch.float32, device="cuda")
    P2.group_points_grad_wrapper(B, C, N, P, S, go, dev(idx), gp)
    got = host(gp)[0]
    del go
    torch.cuda.empty_cache()
    assert np.array_equal(got, want), f"{int((got != want).sum())} wrong elements, channels {np.unique(np.nonzero(got != want)[0])[:8]}"


def test_three_interp_grad_offsets_beyond_2_31():
    """B * C * n = 130 * 2^24 > 2^31 (8.7 GB of grad_out), quarter-integer weights: grad[c, k] = (c + 1) * sum of the weights routed
    to k, exactly."""
    B, C, n, m = 1, 130, 1 << 24, 4096
    assert B * C * n > 2 ** 31
    rng = np.random.default_rng(1)
    idx = rng.integers(0, m, size=(B, n, 3)).astype(np.int32)
    w = (rng.integers(0, 5, size=(B, n, 3)) / 4).astype(np.float32)
    sw = np.bincount(idx.ravel(), weights=w.ravel().astype(np.float64), minlength=m)
    want64 = np.arange(1, C + 1, dtype=np.float64)[:, None] * sw[None, :]
    assert want64.max() < 2 ** 22
    go = torch.arange(1, C + 1, dtype=torch.float32, device="cuda").view(1, C, 1).expand(B, C, n).contiguous()
    gp = torch.zeros((B, C, m), dtype=torch.float32, device="cuda")
    P2.three_interpolate_grad_wrapper(B, C, n, m, go, dev(idx), dev(w), gp)
    got = host(gp)[0]
    del go
    torch.cuda.empty_cache()
    assert np.array_equal(got, want64.astype(np.float32)), f"{int((got != want64).sum())} wrong elements"


# --------------------------------------------------------------------------------------------------------- autograd plumbing
def _plumbing_case(op, rng):
    """(function of features, features shape) with exact-mode-friendly indices."""
    B, C, N = 2, 9, 200
    if op == "group":
        idx = dev(_padded_idx(rng, B, 33, 16, N))
        return (lambda f: PU.grouping_operation(f, idx)), (B, C, N)
    if op == "gather":
        idx = dev(rng.integers(0, N, size=(B, 77)).astype(np.int32))
        return (lambda f: PU.gather_operation(f, idx)), (B, C, N)
    idx = dev(rng.integers(0, N, size=(B, 300, 3)).astype(np.int32))
    w = dev(_weights(rng, (B, 300, 3), True))
    return (lambda f: PU.three_interpolate(f, idx, w)), (B, C, N)


def _grad_of(fn, shape, values, gout=None, loss=None):
    f = torch.tensor(values, device="cuda", requires_grad=True)
    out = fn(f)
    if loss is not None:
        loss(out).backward()
    else:
        out.backward(gout)
    return host(f.grad)


@pytest.mark.parametrize("op", ["group", "gather", "interp"])
def test_grad_out_zero_stride_and_transposed(op):
    """A zero-stride grad_out (out.sum().backward()) and a transposed one give the gradient of their contiguous copies, bit for bit
    (exact mode: integer grads, quarter weights)."""
    rng = np.random.default_rng(40)
    fn, shape = _plumbing_case(op, rng)
    vals = rng.standard_normal(shape).astype(np.float32)
    out_shape = tuple(fn(dev(vals)).shape)
    ones = torch.ones(out_shape, device="cuda")
    assert np.array_equal(_grad_of(fn, shape, vals, loss=lambda o: o.sum()), _grad_of(fn, shape, vals, gout=ones))
    g = dev(rng.integers(-4, 5, size=out_shape[::-1]).astype(np.float32)).permute(*range(len(out_shape) - 1, -1, -1))
    assert g.shape == out_shape and not g.is_contiguous()
    assert np.array_equal(_grad_of(fn, shape, vals, gout=g), _grad_of(fn, shape, vals, gout=g.contiguous()))


def test_grad_out_from_max_pool():
    """The sparse grad_out max-pool backward hands to grouping_operation (SA modules pool every neighbourhood): same gradient as
    its contiguous copy, and equal to the exact scatter-add of it."""
    rng = np.random.default_rng(41)
    B, C, N, P, S = 2, 9, 500, 64, 32
    idx = _padded_idx(rng, B, P, S, N)
    vals = rng.standard_normal((B, C, N)).astype(np.float32)
    W = dev(rng.integers(-4, 5, size=(B, C, P, 1)).astype(np.float32))
    f = torch.tensor(vals, device="cuda", requires_grad=True)
    h = PU.grouping_operation(f, dev(idx))
    (F.max_pool2d(h, kernel_size=[1, S]) * W).sum().backward()
    h2 = h.detach().requires_grad_(True)
    (F.max_pool2d(h2, kernel_size=[1, S]) * W).sum().backward()
    gh = h2.grad
    assert (gh != 0).sum().item() <= B * C * P
    f2 = torch.tensor(vals, device="cuda", requires_grad=True)
    PU.grouping_operation(f2, dev(idx)).backward(gh.contiguous())
    assert np.array_equal(host(f.grad), host(f2.grad))
    _check(host(f.grad), AT.group_grad_exact(host(gh), idx, N), True, "group_grad of a max-pool grad")


@pytest.mark.parametrize("op,shape,ishape", [
    ("group", (0, 3, 10), (0, 4, 5)), ("group", (2, 0, 10), (2, 4, 5)), ("group", (2, 3, 10), (2, 0, 5)),
    ("gather", (0, 3, 10), (0, 4)), ("gather", (2, 0, 10), (2, 4)), ("gather", (2, 3, 10), (2, 0)),
    ("interp", (0, 3, 10), (0, 4, 3)), ("interp", (2, 0, 10), (2, 4, 3)), ("interp", (2, 3, 10), (2, 0, 3))])
def test_empty_shapes_give_zero_gradients(op, shape, ishape):
    f = torch.randn(shape, device="cuda", requires_grad=True)
    idx = torch.zeros(ishape, dtype=torch.int32, device="cuda")
    if op == "group":
        out = PU.grouping_operation(f, idx)
    elif op == "gather":
        out = PU.gather_operation(f, idx)
    else:
        out = PU.three_interpolate(f, idx, torch.full(ishape, 0.25, device="cuda"))
    out.sum().backward()
    torch.cuda.synchronize()
    assert f.grad is not None and f.grad.shape == f.shape and not f.grad.any()


def test_pointnet2_cuda_shim_grad_wrappers_exact():
    """The reference's pointnet2_utils.py calls the *_grad_wrapper functions of the compiled extension directly: one exact-mode case
    per wrapper through the drop-in shim."""
    rng = np.random.default_rng(50)
    B, C, N, P, S = 2, 11, 400, 129, 24
    idx = _padded_idx(rng, B, P, S, N)
    go = _grad_out(rng, (B, C, P, S), True)
    gp = torch.zeros((B, C, N), device="cuda")
    P2.group_points_grad_wrapper(B, C, N, P, S, dev(go), dev(idx), gp)
    _check(host(gp), AT.group_grad_exact(go, idx, N), True, "group_points_grad_wrapper")
    gi = np.ascontiguousarray(idx[:, :, 0])
    go2 = _grad_out(rng, (B, C, P), True)
    gp = torch.zeros((B, C, N), device="cuda")
    P2.gather_points_grad_wrapper(B, C, N, P, dev(go2), dev(gi), gp)
    _check(host(gp), AT.gather_grad_exact(go2, gi, N), True, "gather_points_grad_wrapper")
    i3 = rng.integers(0, N, size=(B, P, 3)).astype(np.int32)
    w = _weights(rng, (B, P, 3), True)
    gp = torch.zeros((B, C, N), device="cuda")
    P2.three_interpolate_grad_wrapper(B, C, P, N, dev(go2), dev(i3), dev(w), gp)
    _check(host(gp), AT.three_interpolate_grad_exact(go2, i3, w, N), True, "three_interpolate_grad_wrapper")


# --------------------------------------------------------------------------------------------- modules and encoder vs float64
def _rel(got, ref):
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    nrm = (g - r).norm().item() / max(r.norm().item(), 1e-300)
    mx = (g - r).abs().max().item() / max(r.abs().max().item(), 1e-300) if r.numel() else 0.0
    return nrm, mx


def _flips(got, ref, tol):
    """Elements off by more than tol * max|ref|: where fp32 and float64 chose different max-pool winners (near-ties)."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    return int(((g - r).abs() > tol * r.abs().max()).sum().item())


def _step(monkeypatch, model, call, inputs, seed):
    """One forward + backward on the HIP route (fp32, train mode) and on the float64 twin replaying its discrete ops.
    inputs: numpy fp32 arrays (each becomes a leaf requiring grad) or None.  The loss is a fixed random weighting of the outputs."""
    twin = AT.Replay.twin(model)
    model = model.cuda()
    rp = AT.Replay(monkeypatch, PU)
    gx = [None if a is None else dev(a).requires_grad_(True) for a in inputs]
    cx = [None if a is None else torch.from_numpy(a).double().requires_grad_(True) for a in inputs]
    with rp.recording():
        outs = call(model, *gx)
    g = torch.Generator().manual_seed(seed)
    Ws = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
    sum((o * W.cuda().float()).sum() for o, W in zip(outs, Ws)).backward()
    with rp.replaying():
        refs = call(twin, *cx)
    sum((o * W).sum() for o, W in zip(refs, Ws)).backward()
    return model, twin, outs, refs, gx, cx


def _compare(model, twin, outs, refs, gx, cx, tol, what):
    """Measured errors against the bounds in `tol`; the measured values are printed (pytest -s) for the record."""
    m = {}
    m["out_rel"] = max(_rel(o, r)[1] for o, r in zip(outs, refs))
    pn, pm = [], []
    for (name, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert (p.grad is None) == (q.grad is None), name
        if q.grad is None:
            continue
        a, b = _rel(p.grad, q.grad)
        pn.append((a, name))
        pm.append((b, name))
    m["param_norm"], m["param_max"] = max(pn)[0], max(pm)[0]
    bn = []
    for (name, b), (_, c) in zip(model.named_buffers(), twin.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(c) == 1, name
        else:
            bn.append(_rel(b, c)[1])
    m["bn_stats"] = max(bn)
    m["input_norm"], m["input_flips"] = 0.0, 0
    for a, c in zip(gx, cx):
        if a is not None:
            assert (a.grad is None) == (c.grad is None)
        if a is not None and a.grad is not None:
            m["input_norm"] = max(m["input_norm"], _rel(a.grad, c.grad)[0])
            m["input_flips"] += _flips(a.grad, c.grad, tol["input_elem"])
    print(f"\nBACKWARD_MEASURED {what} " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in m.items()))
    assert m["out_rel"] <= tol["out_rel"], (what, m)
    assert m["param_norm"] <= tol["param_norm"], (what, m, max(pn))
    assert m["param_max"] <= tol["param_max"], (what, m, max(pm))
    assert m["bn_stats"] <= tol["bn_stats"], (what, m)
    assert m["input_norm"] <= tol["input_norm"], (what, m)
    assert m["input_flips"] <= tol["input_flips"], (what, m)


# Bounds: about 3x the maxima of the first MI355X run (quoted in each test's docstring).  Whole-network gradients differ by more than
# fp32 rounding: where fp32 and float64 pick different max-pool winners (near-ties, and exact ties between the body-like cloud's
# duplicated points), a whole gradient term goes to another element.  Those flips are counted (elements off by more than
# input_elem * max|ref|) and budgeted; the kernels themselves are pinned bit for bit above.
TOL_MODULE = dict(out_rel=2e-6, param_norm=2e-5, param_max=3e-5, bn_stats=1e-6, input_norm=3e-6, input_elem=1e-3, input_flips=0)
TOL_SA_XYZ_ONLY = dict(TOL_MODULE, input_norm=0.1, input_flips=500)
TOL_ENCODER_CFG2 = dict(out_rel=1e-4, param_norm=0.05, param_max=0.3, bn_stats=1e-5, input_norm=0.3, input_elem=1e-3, input_flips=10000)
TOL_ENCODER_GLOBAL = dict(out_rel=2e-3, param_norm=0.15, param_max=0.15, bn_stats=1e-3, input_norm=0.1, input_elem=1e-3,
                          input_flips=20000)


@pytest.mark.parametrize("use_xyz,feats", [(True, False), (True, True), (False, True)], ids=["xyz", "xyz+feats", "feats"])
def test_sa_module_msg_train_step_vs_float64(monkeypatch, use_xyz, feats):
    """Measured on MI355X (max over the three cases): out 4.6e-7, parameter grads norm-wise 3.5e-6 / max-abs 5.4e-6 of max|g_ref|,
    BN running stats 1.1e-7, feature grads 3.1e-7 with no flips.  xyz-only: xyz grads 3.9e-2 norm-wise from 148 flipped elements
    (exact ties between duplicated points of the body-like cloud)."""
    torch.manual_seed(1)
    c = 6 if feats else 0
    sa = PM.PointnetSAModuleMSG(npoint=256, radii=[0.1, 0.2], nsamples=[16, 32], mlps=[[c, 16, 32], [c, 32, 32, 64]],
                                use_xyz=use_xyz).train()
    seed_encoder(sa, seed=2)
    rng = np.random.default_rng(3)
    xyz = syn.body_like_cloud(2, 2048, seed=3)
    f = rng.standard_normal((2, c, 2048)).astype(np.float32) if feats else None
    r = _step(monkeypatch, sa, lambda m, x, ft: m(x, ft), [xyz, f], seed=4)
    _compare(*r, TOL_MODULE if feats else TOL_SA_XYZ_ONLY, f"sa_msg use_xyz={use_xyz} feats={feats}")


@pytest.mark.parametrize("skip", [False, True], ids=["no-skip", "skip"])
def test_fp_module_train_step_vs_float64(monkeypatch, skip):
    """Measured on MI355X: out 4.0e-7, parameter grads 6.4e-7 / 8.1e-7, BN stats 1.1e-7, feature grads 3.0e-7, no flips."""
    torch.manual_seed(5)
    c1, c2 = (16 if skip else 0), 32
    fp = PM.PointnetFPModule(mlp=[c2 + c1, 64, 32]).train()
    seed_encoder(fp, seed=6)
    rng = np.random.default_rng(7)
    unknown = syn.body_like_cloud(2, 2048, seed=7)
    known = np.ascontiguousarray(unknown[:, rng.permutation(2048)[:256]])
    uf = rng.standard_normal((2, c1, 2048)).astype(np.float32) if skip else None
    kf = rng.standard_normal((2, c2, 256)).astype(np.float32)
    r = _step(monkeypatch, fp, lambda m, u, k, a, b: (m(u, k, a, b),), [unknown, known, uf, kf], seed=8)
    _compare(*r, TOL_MODULE, f"fp skip={skip}")


def _encoder_call(model, pc):
    middle, logits, _, _ = model(pc)
    return (logits,) if middle is None else (logits, middle)


@pytest.mark.parametrize("kind", ["unit", "body"])
def test_encoder_cfg2_train_step_vs_float64(monkeypatch, kind):
    """Pointnet2MSGSEG(input_channels=0, global_feat=False) at cfg2 size (B = 8, N = 8192).
    Measured on MI355X (max of unit / body): logits 1.7e-5, parameter grads norm-wise 1.7e-2 / max-abs 9.2e-2, BN stats 2.2e-6,
    xyz grads 9.9e-2 norm-wise with 3711 of 196608 elements flipped."""
    model = seed_encoder(Pointnet2MSGSEG(input_channels=0, global_feat=False), seed=9).train()
    model.FC_layer[1].eval()                          # dropout off: the twin cannot replay its random mask
    cloud = syn.unit_cloud if kind == "unit" else syn.body_like_cloud
    r = _step(monkeypatch, model, _encoder_call, [cloud(8, 8192, seed=10)], seed=11)
    _compare(*r, TOL_ENCODER_CFG2, f"encoder cfg2 {kind}")


def test_encoder_with_features_and_global_feat_train_step_vs_float64(monkeypatch):
    """Pointnet2MSGSEG(input_channels=3, global_feat=True) at N = 6890 with the input features requiring grad; the loss also weights
    the global (middle) features so that the GroupAll module is trained too.
    Measured on MI355X: outputs 4.0e-4 (the GroupAll MLP normalises over B = 2 rows), parameter grads 4.4e-2 / 4.9e-2, BN stats
    2.8e-4, input grads 2.8e-2 norm-wise with 7535 of 82680 elements flipped."""
    model = seed_encoder(Pointnet2MSGSEG(input_channels=3, global_feat=True), seed=12).train()
    model.FC_layer[1].eval()
    rng = np.random.default_rng(13)
    pc = np.concatenate([syn.body_like_cloud(2, 6890, seed=13), rng.standard_normal((2, 6890, 3)).astype(np.float32)], axis=2)
    r = _step(monkeypatch, model, _encoder_call, [np.ascontiguousarray(pc)], seed=14)
    _compare(*r, TOL_ENCODER_GLOBAL, "encoder N=6890 input_channels=3 global_feat")
