"""Set-form neighbour lists (g4d_ball_grid_query_set_f32, csrc/ball_grid.hip): per (query, scale) the SAME SET of indices as the ordered
entry point g4d_ball_grid_query_f32 -- which the existing tests pin to the oracle bit for bit -- each index once among the leading slots,
in any order, every remaining slot a copy of slot 0, rows without a hit all zero.  And the consumers: a max-pooled fused SA level gives
the same bits with either form, an average-pooled one keeps the ordered lists."""
import numpy as np
import pytest
import torch

from garment4d_amd import _lib, fused, pointnet2_modules as PM, synthetic as syn, tuning as T

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("contraction_mode")]

B, N, P = 2, 1500, 37
RADII, NS = (0.05, 0.1), (16, 32)
# special queries 0 .. 7: (centre, points placed around it as (count, shortest, longest distance from the centre, duplicated))
CENTRES = np.array([[50, 50, 50], [0.2, 0.2, 0.2], [0.8, 0.2, 0.2], [0.2, 0.8, 0.2], [0.8, 0.8, 0.2], [0.2, 0.2, 0.8], [0.8, 0.2, 0.8], [0.2, 0.8, 0.8]], np.float32)
SHELLS = {1: [(5, 0.0, 0.03, False)],                                   # fewer hits than slots at both scales
          2: [(16, 0.0, 0.04, False), (16, 0.06, 0.09, False)],         # exactly nsample hits: 16 | 32
          3: [(17, 0.0, 0.04, False), (16, 0.06, 0.09, False)],         # nsample + 1 hits: 17 | 33
          4: [(300, 0.0, 0.04, False)],                                 # 65 .. 512 hits: the list spans several registers per lane
          5: [(700, 0.0, 0.04, False)],                                 # more than kCap = 512 hits: the dense fallback
          6: [(6, 0.0, 0.03, True)]}                                    # duplicated points: 12 hits at 6 places
WANT_HITS = {0: (0, 0), 1: (5, 5), 2: (16, 32), 3: (17, 33), 4: (300, 300), 5: (700, 700), 6: (12, 12), 7: (0, 0)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_case():
    """(xyz (B,N,3), queries (B,P,3)): the special neighbourhoods above in a sparse background that keeps 0.25 away from their centres, the
    points in shuffled order (so that arrival order in a cell is not index order); every intended case asserted here, on the host."""
    rng = np.random.default_rng(11)
    xyz = np.empty((B, N, 3), np.float32)
    q = np.empty((B, P, 3), np.float32)
    for b in range(B):
        pts = []
        for k, shells in SHELLS.items():
            for cnt, r0, r1, dup in shells:
                d = rng.standard_normal((cnt, 3))
                d /= np.linalg.norm(d, axis=1, keepdims=True)
                p = CENTRES[k] + d * rng.uniform(r0 + 1e-3, r1 - 1e-3, (cnt, 1))
                pts.append(np.concatenate([p, p]) if dup else p)
        pts = np.concatenate(pts)
        bg = np.empty((0, 3))
        while len(bg) < N - len(pts):
            c = rng.uniform(0, 1, (4 * N, 3))
            bg = np.concatenate([bg, c[(np.linalg.norm(c[:, None] - CENTRES[None, 1:], axis=2) > 0.25).all(1)]])
        cloud = np.concatenate([pts, bg[:N - len(pts)]]).astype(np.float32)
        xyz[b] = cloud[rng.permutation(N)]
        q[b, :8] = CENTRES
        q[b, 7, 1] = np.nan                                            # a NaN query coordinate
        q[b, 8:] = xyz[b, rng.integers(0, N, P - 8)] + rng.standard_normal((P - 8, 3)).astype(np.float32) * 0.02
    dist = np.linalg.norm(xyz[:, None].astype(np.float64) - q[:, :, None].astype(np.float64), axis=3)   # (B, P, N)
    for k, want in WANT_HITS.items():
        for r, w in zip(RADII, want):
            if k != 7:
                assert np.abs(dist[:, k] - r).min() > 1e-4             # no hit is decided by rounding
            assert ((dist[:, k] < r).sum(1) == w).all(), (k, r)
    assert all(len(np.unique(xyz[b], axis=0)) == N - 6 for b in range(B))
    return xyz, q


@pytest.fixture(scope="module")
def case():
    return make_case()


def check_set_form(ordered, sets):
    for o, s in zip(ordered, sets):
        o, s = o.cpu().numpy(), s.cpu().numpy()
        assert o.shape == s.shape
        for ro, rs in zip(o.reshape(-1, o.shape[-1]), s.reshape(-1, s.shape[-1])):
            members = set(ro.tolist())
            k = len(members)
            assert set(rs.tolist()) == members
            assert sorted(rs[:k].tolist()) == sorted(members)          # each index once among the first len(set) slots
            assert (rs[k:] == rs[0]).all()                             # padding repeats slot 0
            assert (ro == 0).all() == (rs == 0).all()


@pytest.mark.parametrize("radii,ns", [(RADII, NS), ((0.03, 0.05, 0.08, 0.1), (8, 16, 24, 32))], ids=["two-scales", "four-scales"])
def test_set_form_holds_the_ordered_form_sets(case, radii, ns):
    xyz, q = case
    x, qd = dev(xyz), dev(q)
    grid = fused.build_ball_grid(x, max(radii))
    ordered = fused.ball_query_msg(radii, ns, x, qd, grid=grid)
    sets = fused.ball_query_msg(radii, ns, x, qd, grid=grid, set_form=True)
    if radii == RADII:   # the ordered lists show the cases the host arranged
        for k, want in WANT_HITS.items():
            for o, w, n_ in zip(ordered, want, ns):
                rows = o[:, k].cpu().numpy()
                assert all(len(set(r.tolist())) == max(1, min(w, n_)) for r in rows), (k, w)
                assert w > 0 or (rows == 0).all()
    check_set_form(ordered, sets)
    scan = fused.ball_query_msg(radii, ns, x, qd, grid=False, set_form=True)   # the keyword leaves the other routes alone
    assert all(torch.equal(a, b_) for a, b_ in zip(ordered, scan))


def _seed_bn(mod):
    for m in mod.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.1)
    return mod.cuda().eval()


def _calls(monkeypatch):
    names = []
    real = _lib.call

    def call(name, *a, **kw):
        names.append(name)
        return real(name, *a, **kw)
    monkeypatch.setattr(_lib, "call", call)
    return names


def _on_off(sa, xyz, fpm, grid, native=None):
    outs = []
    with torch.no_grad():
        for on in (True, False):
            with T.use(T.current().replace(bq_set=on, native=native or {})):
                outs.append(fused.sa_forward(sa, xyz, fpm, grid=grid)[1])
    return outs


def test_xyz_pair_kernel_gives_the_same_bits(monkeypatch):
    """The encoder's first level (csrc/sa_xyz.hip, both scales in one launch) over set-form and over ordered lists."""
    torch.manual_seed(3)
    xyz = dev(syn.unit_cloud(2, 4096, seed=5))
    sa = _seed_bn(PM.PointnetSAModuleMSG(npoint=64, radii=[0.05, 0.1], nsamples=[16, 32], mlps=[[0, 16, 16, 32], [0, 32, 32, 64]]))
    names = _calls(monkeypatch)
    on, off = _on_off(sa, xyz, None, None)
    assert torch.equal(on, off)
    assert names.count("g4d_ball_grid_query_set_f32") == 1 and names.count("g4d_ball_grid_query_f32") == 1
    assert names.count("g4d_sa_xyz_mlp3_pair_f32") == 2


def test_table_kernel_with_dead_tiles_gives_the_same_bits(monkeypatch):
    """A level with features on sa_table.hip's persistent kernel, S = 32, small balls (about 14 of 600 points): many second tiles are padding, which the kernel
    recognises by comparing with slot 0 -- the padding rule of the set form."""
    torch.manual_seed(4)
    xyz = dev(syn.unit_cloud(2, 600, seed=6))
    fpm = torch.randn(2, 600, 40, device="cuda")
    sa = _seed_bn(PM.PointnetSAModule(npoint=77, radius=0.18, nsample=32, mlp=[40, 64, 64, 128]))
    names = _calls(monkeypatch)
    on, off = _on_off(sa, xyz, fpm, True, native={"sa_table_persistent": 1, "sa_table_min_rows": 0})
    assert torch.equal(on, off)
    assert names.count("g4d_ball_grid_query_set_f32") == 1 and names.count("g4d_ball_grid_query_f32") == 1
    assert names.count("g4d_mlp_chain_group_table_ws_f32") == 2
    idx = fused.ball_query_msg([0.18], [32], xyz, fused.fps_gather(xyz, 77), grid=True)[0]
    dead = (idx[..., 16:] == idx[..., :1]).all(-1)
    assert dead.any() and not dead.all()                               # neighbourhoods with a dead second tile, and others


def test_avg_pool_keeps_the_ordered_lists(monkeypatch):
    torch.manual_seed(5)
    xyz = dev(syn.unit_cloud(2, 600, seed=7))
    fpm = torch.randn(2, 600, 40, device="cuda")
    sa = _seed_bn(PM.PointnetSAModule(npoint=77, radius=0.12, nsample=32, mlp=[40, 64, 64, 128], pool_method="avg_pool"))
    names = _calls(monkeypatch)
    on, off = _on_off(sa, xyz, fpm, True)
    assert torch.equal(on, off)
    assert names.count("g4d_ball_grid_query_f32") == 2 and "g4d_ball_grid_query_set_f32" not in names
