"""The bucketed sampling kernel (csrc/fps_bucket.hip) orders the cloud with a counting sort on a coarse Morton cell; the place of a point
within its cell is up to the order in which LDS atomics retire.  The outputs may not be: samples, gathered coordinates and the reference's
scratch against the oracle, in both distance-contraction modes, through g4d_fps_gather_grid_f32 and the plain entry point, on clouds
that put everything into one cell, none into most, or non-finite coordinates into the box -- each case twice, the runs compared."""
import numpy as np
import pytest
import torch

from garment4d_amd import _lib, fused, pointnet2_cuda as shim, synthetic as syn
from oracle import pointnet2_oracle as K

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("contraction_mode")]

B = 3


def _cloud(kind, n, b=B):
    rng = np.random.default_rng(n + len(kind))
    x = syn.unit_cloud(b, n, seed=n + 1)
    if kind == "identical":
        x[:] = np.float32(0.37)
    elif kind == "one-cell":        # distinct points, but one outlier stretches the extent: every other point falls into the first cell
        x[:, 17] = 1e6
    elif kind == "line":
        x = np.zeros((b, n, 3), np.float32)
        for i in range(b):
            x[i, :, 0] = rng.permutation(np.linspace(0, 1, n, dtype=np.float32))
    elif kind == "nonfinite":
        x[:, 100, 1] = np.nan
        x[:, 200, 2] = np.inf
    return np.ascontiguousarray(x)


CASES = [("uniform", 4097, 64), ("uniform", 5000, 64), ("uniform", 8192, 1024), ("identical", 8192, 64), ("one-cell", 8192, 64), ("line", 8192, 64),
         ("nonfinite", 8192, 64)]
_want = {}


def want(kind, n, m, mode, b=B):
    """The oracle's (samples, scratch) for a case in the contraction mode in force: computed once, shared, read only."""
    key = (kind, n, m, mode, b)
    if key not in _want:
        idx, temp = K.fps(_cloud(kind, n, b), m, return_temp=True)
        idx.setflags(write=False); temp.setflags(write=False)
        _want[key] = (idx, temp)
    return _want[key]


def run_plain(xd, m):
    b, n, _ = xd.shape
    temp = torch.full((b, n), 1e10, device="cuda")
    idx = torch.empty((b, m), dtype=torch.int32, device="cuda")
    shim.furthest_point_sampling_wrapper(b, n, m, xd, temp, idx)
    return idx.cpu().numpy(), temp.cpu().numpy()


def run_grid(xd, m):
    b, n, _ = xd.shape
    idx = torch.empty((b, m), dtype=torch.int32, device="cuda")
    nx = torch.empty((b, m, 3), dtype=torch.float32, device="cuda")
    ws = _lib.workspace(_lib.lib().g4d_ball_grid_bytes(b, n), xd.device)
    _lib.call("g4d_fps_gather_grid_f32", b, n, m, xd.data_ptr(), idx.data_ptr(), nx.data_ptr(), 0.1, ws.data_ptr(), _lib.stream_ptr())
    return idx.cpu().numpy(), nx.cpu().numpy()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("kind,n,m", CASES, ids=[f"{k}-{n}-{m}" for k, n, m in CASES])
def test_samples_coordinates_and_scratch_are_exact_and_repeatable(kind, n, m, contraction_mode):
    x = _cloud(kind, n)
    w_idx, w_temp = want(kind, n, m, contraction_mode)
    w_nx = np.take_along_axis(x, w_idx[..., None].astype(np.int64), 1)
    xd = torch.from_numpy(x).cuda()
    plain = [run_plain(xd, m) for _ in range(2)]
    grid = [run_grid(xd, m) for _ in range(2)]
    for idx, temp in plain:
        assert np.array_equal(idx, w_idx), f"first mismatch at {np.argwhere(idx != w_idx)[:3]}"
        assert same(temp, w_temp)
    for idx, nx in grid:
        assert np.array_equal(idx, w_idx), f"first mismatch at {np.argwhere(idx != w_idx)[:3]}"
        assert same(nx, w_nx)
    assert same(plain[0][1], plain[1][1]) and same(grid[0][1], grid[1][1])
    assert same(fused.fps_gather(xd, m).cpu().numpy(), w_nx)


def test_register_form_of_the_coalesced_calls(contraction_mode):
    """32 clouds in one call: the launch takes the register form of the round loop (no LDS copy of the cloud), the executor's regime."""
    b, n, m = 32, 8192, 64
    x = _cloud("uniform", n, b)
    w_idx, w_temp = want("uniform", n, m, contraction_mode, b)
    xd = torch.from_numpy(x).cuda()
    for _ in range(2):
        idx, nx = run_grid(xd, m)
        assert np.array_equal(idx, w_idx) and same(nx, np.take_along_axis(x, w_idx[..., None].astype(np.int64), 1))
        idx, temp = run_plain(xd, m)
        assert np.array_equal(idx, w_idx) and same(temp, w_temp)
