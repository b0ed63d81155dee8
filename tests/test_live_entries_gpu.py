"""The live-cloud scope (include/g4d_live.h) at every converted entry point of the hot path: launched on `cap` clouds inside a scope whose
device-side count is `live`, an entry point must

  * give the first `live` clouds the BITS of the same entry point launched on b = live clouds without a scope, and
  * leave every output row of the other clouds alone: the outputs (and every buffer the wrappers of fused.py / lbs.py allocate on the way)
    are filled with a sentinel bit pattern beforehand, and the dead clouds' rows must still hold it afterwards -- which shows that the work
    is skipped without timing anything.

live runs over {0, 1, cap - 1, cap}; the persistent kernels are reached at small shapes through the tuning keys, as in
tests/test_large_launch_gpu.py.  The shapes put the live boundary inside a pass / tile / block wherever the kernel has one: clouds of 63 or
21 neighbourhoods, 300 or 1000 rows, 4100 points.

The sentinels: float32 buffers hold the NaN 0x7fc0dead; int32 buffers (neighbour indices) hold 1 -- a valid index for every cloud here, so
that a kernel which did read a dead cloud's list would still stay inside its arrays; scratch bytes hold 0."""
import contextlib

import pytest
import torch

from garment4d_amd import _lib, fused, lbs as L, pointnet2_modules as PM, pytorch_utils as pt_utils, synthetic as syn

pytestmark = pytest.mark.gpu

CAP = 4
LIVES = (0, 1, CAP - 1, CAP)
SENT_F, SENT_I = 0x7fc0dead, 1


def tuning(**kv):
    from garment4d_amd import tuning as T
    return T.use(T.current().replace(native=kv))


def _fill(t):
    if t.dtype == torch.float32:
        t.view(torch.int32).fill_(SENT_F)
    elif t.dtype == torch.int32:
        t.fill_(SENT_I)
    elif t.dtype == torch.uint8:
        t.zero_()
    return t


@contextlib.contextmanager
def sentinel_allocations():
    """torch.empty, as the wrappers call it, hands out sentinel-filled tensors inside the block."""
    real = torch.empty

    def empty(*a, **kw):
        return _fill(real(*a, **kw))

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def scoped(live, fn, cap=CAP):
    """fn() with sentinel allocations inside a scope of `cap` clouds whose count is `live`."""
    cnt = torch.tensor([live], dtype=torch.int32, device="cuda")
    with torch.no_grad(), sentinel_allocations(), _lib.live_scope(cnt, cap):
        out = fn()
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def check(got, want, live, what, cap=CAP, canon=None):
    """got: an output over `cap` clouds (leading dimension cap, or cap * rows-per-cloud rows); want: the same over the first `live` clouds."""
    g = bits(got).reshape(cap, -1)
    if live:
        w = bits(want).reshape(live, -1)
        a, b = (g[:live], w) if canon is None else (canon(got[:live]), canon(want))
        assert torch.equal(a, b), f"{what}: live clouds differ at live = {live}"
    sent = SENT_F if got.dtype == torch.float32 else (SENT_I if got.dtype == torch.int32 else 0)
    assert bool((g[live:] == sent).all()), f"{what}: {int((g[live:] != sent).sum())} elements of dead clouds were written at live = {live}"
    if live and got.dtype != torch.uint8:
        assert not bool((g[:live] == sent).all(1).any()), f"{what}: a live cloud was left untouched at live = {live}"


def run_lives(fn, names, canon=None, cap=CAP, lives=None):
    """fn(b) -> tuple of outputs of the entry point on the first b clouds.  For every live count: unscoped on b = live first (the reference; it
    also packs the weights outside the sentinel block), then on b = cap inside the scope."""
    with torch.no_grad():
        fn(cap)   # (once without a scope: packs weights, sets kernel attributes)
    for live in (lives or (0, 1, cap - 1, cap)):
        with torch.no_grad():
            want = fn(live) if live else None
        got = scoped(live, lambda: fn(cap), cap)
        for i, name in enumerate(names):
            check(got[i], None if want is None else want[i], live, name, cap, canon)


def _seed_bn(mod):
    for m in mod.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.1)
    return mod.cuda().eval()


@pytest.fixture(autouse=True)
def _module_forward_is_op_by_op():
    with PM.op_by_op():
        yield


@pytest.fixture(scope="module")
def cloud():
    """4 clouds of 4100 points (more than 4096: the sampling launch that also builds the cell grids) and their 64 / 63 centres, computed once."""
    xyz = torch.from_numpy(syn.unit_cloud(CAP, 4100, seed=11)).cuda()
    return xyz, fused.fps_gather(xyz, 64), fused.fps_gather(xyz, 63)


# ---- sampling launches: one workgroup per cloud -------------------------------------------------------------------------------------------

def test_fps_gather_grid(cloud):
    """g4d_fps_gather_grid_f32: the sampling workgroup AND the grid-building workgroup of a dead cloud leave at once."""
    xyz = cloud[0]

    def fn(b):
        nx, (ws, _) = fused.fps_gather_grid(xyz[:b], 64, 0.2)
        return nx, ws
    for live in LIVES:
        want = fn(live) if live else None
        nx, ws = scoped(live, lambda: fn(CAP))
        check(nx, None if want is None else want[0], live, "new_xyz")
        per = ws.numel() // CAP
        assert ws.numel() == per * CAP and bool((ws.view(CAP, per)[live:] == 0).all()), "grid of a dead cloud was built"
        assert all(bool((ws.view(CAP, per)[c] != 0).any()) for c in range(live)), "grid of a live cloud is missing"
        if live:   # the grids serve the ball query: same lists as on b = live clouds
            idx = fused.ball_query_msg([0.1, 0.2], [16, 32], xyz[:live], nx[:live], grid=(ws[:per * live], 0.2))
            ref = fused.ball_query_msg([0.1, 0.2], [16, 32], xyz[:live], want[0], grid=(want[1], 0.2))
            assert all(torch.equal(a, b) for a, b in zip(idx, ref))


def test_fps_gather_pair(cloud):
    x = fused.fps_gather(cloud[0], 1024)
    run_lives(lambda b: fused.fps_gather_pair(x[:b], 256, 64), ("new_xyz1", "new_xyz2"))


# ---- searches ----------------------------------------------------------------------------------------------------------------------------

def test_search_multi(cloud):
    """g4d_search_multi_f32: the ball queries of SA 2 / 3 and the inner three-NN searches in one launch."""
    n0 = fused.fps_gather(cloud[0], 1024)
    n1, n2 = fused.fps_gather_pair(n0, 256, 64)

    def fn(b):
        o0, o1, nn = fused.search_multi(([0.2, 0.4], [16, 32], n0[:b], n1[:b]), ([0.4, 0.8], [32, 64], n1[:b], n2[:b]),
                                        [(n1[:b], n2[:b]), (n0[:b], n1[:b])])
        return (*o0, *o1, nn[0][0], nn[0][1], nn[1][0], nn[1][1])
    run_lives(fn, ("idx0[0]", "idx0[1]", "idx1[0]", "idx1[1]", "dist2 a", "nn_idx a", "dist2 b", "nn_idx b"))


@pytest.mark.parametrize("set_form", [False, True])
def test_ball_grid_query(cloud, set_form):
    """g4d_ball_grid_query_f32 / g4d_ball_grid_query_set_f32 (the set form's lists are sets: compared sorted)."""
    xyz, nx, _ = cloud
    grid = fused.build_ball_grid(xyz, 0.2)
    per = grid[0].numel() // CAP

    def fn(b):
        return tuple(fused.ball_query_msg([0.1, 0.2], [16, 32], xyz[:b], nx[:b], grid=(grid[0][:per * b], 0.2), set_form=set_form))
    run_lives(fn, ("idx r=0.1", "idx r=0.2"), canon=(lambda t: t.sort(-1)[0]) if set_form else None)


def test_three_nn_pruned(cloud):
    """g4d_three_nn_pruned_f32: pre-pass and search, queries in index order and in the cell order of the unknown cloud's grid."""
    xyz = cloud[0]
    known = fused.fps_gather(xyz, 300)
    grid = fused.build_ball_grid(xyz, 0.2)
    per = grid[0].numel() // CAP
    for use_grid in (False, True):
        def fn(b):
            d = torch.empty((b, 4100, 3), dtype=torch.float32, device="cuda")
            i = torch.empty((b, 4100, 3), dtype=torch.int32, device="cuda")
            fused.three_nn_pruned(xyz[:b], (grid[0][:per * b], 0.2) if use_grid else None, known[:b], d, i, sorted_out=False)
            return d, i
        run_lives(fn, ("dist2", "nn_idx"))


# ---- set abstraction ---------------------------------------------------------------------------------------------------------------------

def test_sa_xyz_pair(cloud):
    """g4d_sa_xyz_mlp3_pair_f32 behind the set-form grid query: 63 centres per cloud, so the live boundary falls inside a 32-row pass of the
    16-sample scale."""
    xyz, _, nx = cloud
    grid = fused.build_ball_grid(xyz, 0.2)
    per = grid[0].numel() // CAP
    torch.manual_seed(1)
    sa = _seed_bn(PM.PointnetSAModuleMSG(npoint=63, radii=[0.1, 0.2], nsamples=[16, 32], mlps=[[0, 16, 16, 32], [0, 32, 32, 64]]))
    run_lives(lambda b: (fused.sa_forward(sa, xyz[:b], None, new_xyz=nx[:b], grid=(grid[0][:per * b], 0.2))[1],), ("SA 1 features",))


@pytest.mark.parametrize("N,P,C,mlps,nsamples", [
    (256, 63, 96, [[96, 32, 32, 64], [96, 64, 64, 128]], [16, 32]),       # SA 2: sa_table_kernel<32,16> and <64,32>; the table: linear_kernel
    (128, 21, 192, [[192, 64, 64, 128], [192, 128, 128, 256]], [32, 64]),  # SA 3: <64,32> and the lock-step stack <128,64,1,2> with its work list;
                                                                           #   21 and 63 live neighbourhoods: the boundary inside a round of four
    (128, 16, 192, [[192, 64, 64, 128], [192, 128, 128, 256]], [32, 64]),  # ... and on a round boundary
])
def test_sa_table_levels(N, P, C, mlps, nsamples):
    """g4d_linear_f32 (the first-layer table) + g4d_mlp_chain_group_table_ws_f32 per scale, on the persistent kernels."""
    torch.manual_seed(N + P)
    xyz = torch.from_numpy(syn.unit_cloud(CAP, N, seed=N)).cuda()
    fpm = torch.randn(CAP, N, C, device="cuda")
    nx = fused.fps_gather(xyz, P)
    sa = _seed_bn(PM.PointnetSAModuleMSG(npoint=P, radii=[0.25, 0.4], nsamples=nsamples, mlps=[list(m) for m in mlps]))
    idxs = fused.ball_query_msg([0.25, 0.4], nsamples, xyz, nx)
    with tuning(sa_table_min_rows=0):
        assert int(_lib.lib().g4d_sa_table_supported(CAP * P * nsamples[1], mlps[1][1], nsamples[1], 1)) == 1
        run_lives(lambda b: (fused.sa_forward(sa, xyz[:b], fpm[:b], new_xyz=nx[:b], idxs=[i[:b] for i in idxs])[1],), ("SA features",))
        with tuning(sa_table_persistent=0):   # the same bits as the chain kernels, which ignore the scope and compute every cloud
            ref = fused.sa_forward(sa, xyz, fpm, new_xyz=nx, idxs=idxs)[1]
        cnt = torch.tensor([CAP], dtype=torch.int32, device="cuda")
        with torch.no_grad(), _lib.live_scope(cnt, CAP):
            assert torch.equal(fused.sa_forward(sa, xyz, fpm, new_xyz=nx, idxs=idxs)[1], ref)


# ---- GEMMs -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per,K,Cout,native", [
    (300, 192, 192, {}),                                   # linear_kernel (SA 3's table): 64-row blocks, the boundary inside one
    (300, 256, 256, {"gemm_tile_min_rows": 0}),            # gemm_tile_kernel: 128 x 128 tiles, row blocks numbered in groups of 8
    (1100, 512, 384, {"gemm_tile_min_rows": 0}),           # ... 35 row blocks x 3 column blocks: more than one group of 8, live groups 0-1, 0-7
    (8200, 96, 96, {}),                                    # gemm_narrow_kernel (SA 2's table; taken from 32768 rows on)
])
def test_linear(per, K, Cout, native):
    """g4d_linear_f32: rows only -- the scope applies because the rows are a multiple of its capacity."""
    g = torch.Generator().manual_seed(per)
    x = torch.randn(CAP * per, K, generator=g).cuda()
    layer = fused.PackedLayer((torch.randn(Cout, K, generator=g) / K ** 0.5).cuda(), (torch.rand(Cout, generator=g) + 0.5).cuda(),
                              torch.randn(Cout, generator=g).cuda(), relu=True)
    with tuning(**native):
        run_lives(lambda b: (fused.linear(x[:b * per], layer),), ("linear output",))
        # rows that are NOT a multiple of the capacity: the launch ignores the scope and computes everything
        cnt = torch.tensor([1], dtype=torch.int32, device="cuda")
        with _lib.live_scope(cnt, CAP):
            got = fused.linear(x[:CAP * per - 1], layer)
        assert torch.equal(got, fused.linear(x[:CAP * per - 1], layer))


def test_count_is_clamped_to_the_capacity():
    """A count above the capacity is the capacity, a negative one is 0: never a row past the launch's own."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(CAP * 300, 192, generator=g).cuda()
    layer = fused.PackedLayer((torch.randn(192, 192, generator=g) / 14).cuda(), torch.ones(192).cuda(), torch.zeros(192).cuda(), relu=False)
    want = fused.linear(x, layer)
    check(scoped(CAP + 5, lambda: fused.linear(x, layer)), want, CAP, "count above the capacity")
    check(scoped(-3, lambda: fused.linear(x, layer)), None, 0, "negative count")


# ---- feature propagation -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("native", [{}, {"gemm_tile_min_rows": 0}])
def test_linear_interp_add(native):
    """g4d_linear_interp_add_f32 (the wide FP level: [384 + 192 -> 512 -> 256] over 300 points per cloud) on linear_kernel and on gemm_tile_kernel,
    with the g4d_linear_f32 launches around it."""
    torch.manual_seed(3)
    n, m = 300, 64
    unknown = torch.from_numpy(syn.unit_cloud(CAP, n, seed=n)).cuda()
    known = fused.fps_gather(unknown, m)
    kf, skip = torch.randn(CAP, m, 384, device="cuda"), torch.randn(CAP, n, 192, device="cuda")
    fp = _seed_bn(PM.PointnetFPModule(mlp=[576, 512, 256]))
    nn = fused.three_nn(unknown, known)
    with tuning(**native):
        with torch.no_grad(), _lib.timed_calls() as t:
            fused.fp_forward(fp, unknown, known, skip, kf, nn=nn)
        assert "g4d_linear_interp_add_f32" in [name for name, _, _ in t.results()]
        run_lives(lambda b: (fused.fp_forward(fp, unknown[:b], known[:b], skip[:b], kf[:b], nn=(nn[0][:b], nn[1][:b])),), ("FP 3 features",))


def test_fp_init():
    """g4d_mlp_chain_interp_init_f32 (FP 2 + FP 1's table) on fp_init_kernel; 1000 points per cloud: tiles straddle clouds."""
    torch.manual_seed(5)
    n, m = 1000, 100
    unknown = torch.from_numpy(syn.unit_cloud(CAP, n, seed=n)).cuda()
    known = fused.fps_gather(unknown, m)
    kf, skip = torch.randn(CAP, m, 256, device="cuda"), torch.randn(CAP, n, 96, device="cuda")
    fp = _seed_bn(PM.PointnetFPModule(mlp=[352, 256, 128]))
    raw = fused.fp_table_layer(_seed_bn(PM.PointnetFPModule(mlp=[128, 128, 64])), 0, 128, None)
    nn = fused.three_nn(unknown, known)
    with tuning(fp_init_min_rows=0):
        run_lives(lambda b: fused.fp_forward(fp, unknown[:b], known[:b], skip[:b], kf[:b], nn=(nn[0][:b], nn[1][:b]), also_table=raw),
                  ("FP 2 features", "FP 1 table"))


@pytest.mark.parametrize("cells", [True, False])
def test_fp_table_head(cloud, cells, tune):
    """g4d_mlp_chain_table_cells_f32 / g4d_mlp_chain_table_f32 (FP 1 + head) on fp_table_head_kernel; 4100 points per cloud: tiles straddle clouds."""
    torch.manual_seed(7)
    unknown = cloud[0]
    known = fused.fps_gather(unknown, 257)
    kf = torch.randn(CAP, 257, 128, device="cuda")
    fp = _seed_bn(PM.PointnetFPModule(mlp=[128, 128, 64]))
    head = _seed_bn(torch.nn.Sequential(pt_utils.Conv1d(64, 32, bn=True), torch.nn.Dropout(), pt_utils.Conv1d(32, 7, activation=None)))
    grid = fused.build_ball_grid(unknown, 0.1)
    per = grid[0].numel() // CAP
    tune(fp_cells=cells)
    with tuning(fp_table_min_rows=0):
        run_lives(lambda b: fused.fp_forward(fp, unknown[:b], known[:b], None, kf[:b], head=head, unknown_grid=(grid[0][:per * b], 0.1)),
                  ("FP 1 features", "logits"))


# ---- lbs(): frames counted as clouds -----------------------------------------------------------------------------------------------------

def test_lbs_mfma():
    """g4d_lbs_mfma_f32, both kernels: 3 frames of one 16-frame tile; the vertex count is not a multiple of the 32-vertex tile."""
    P = {k: torch.from_numpy(v).cuda() for k, v in syn.smpl_like_params(seed=3).items()}
    assert P["v_template"].shape[0] % 32 != 0
    betas, pose = (torch.from_numpy(a).cuda() for a in syn.smpl_like_pose(3, seed=3))
    args = (P["v_template"], P["shapedirs"], P["posedirs"], P["J_regressor"], P["parents"], P["lbs_weights"])
    run_lives(lambda b: L.lbs(betas[:b], pose[:b], *args), ("verts", "joints"), cap=3)
