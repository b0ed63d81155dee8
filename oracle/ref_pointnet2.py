"""ctypes front-end of the reference build: oracle/_ref/libpointnet2_ref.so (`make -C oracle ref`, oracle/ref_entry.hip).

TEST INFRASTRUCTURE ONLY -- loaded by tests/test_ref_kernels_gpu.py and scripts/dump_ref_kernels.py; never by garment4d_amd/,
smoke() or bench.py.  The library is the reference's own four pointnet2 kernel files compiled for gfx950 with -ffp-contract=off;
this module only loads what `make ref` left behind and never reads the reference's directory.

The nine `*_wrapper` functions have the signatures of the reference's pointnet2_api.cpp -- the same ones
`oracle.pointnet2_oracle.as_pointnet2_cuda_module()` (CPU tensors) and `garment4d_amd.pointnet2_cuda` (the product) have, so the
three are interchangeable modules.  Device torch tensors, in-place outputs, torch's current stream.

The reference's kernels check nothing: an empty grid is a launch error that ends the process (its launchers call exit()), an index
outside its array is an out-of-bounds access.  The wrappers here therefore refuse (ValueError) a zero dimension, a tensor smaller
than the dimensions say, and an index tensor with an entry outside [0, n) -- before anything is launched.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libpointnet2_ref.so")
_lib = None

_I, _F, _P = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
_PROTOTYPES = {
    "g4d_ref_opt_n_threads": (_I, [_I]),
    "g4d_ref_fps": (None, [_I, _I, _I, _P, _P, _P, _P]),
    "g4d_ref_gather": (None, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "g4d_ref_gather_grad": (None, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "g4d_ref_ball_query": (None, [_I, _I, _I, _F, _I, _P, _P, _P, _P]),
    "g4d_ref_group": (None, [_I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "g4d_ref_group_grad": (None, [_I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "g4d_ref_three_nn": (None, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "g4d_ref_three_interp": (None, [_I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "g4d_ref_three_interp_grad": (None, [_I, _I, _I, _I, _P, _P, _P, _P, _P]),
}


def available():
    """True when `make -C oracle ref` (run by __graft_entry__.build() where a reference checkout is at hand) has left the library."""
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `G4D_REFERENCE_DIR=<checkout of the reference> make -C oracle ref`")
        import torch  # noqa: F401  torch first, so that its HIP runtime is the only one in the process (see garment4d_amd/_lib.py)
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def opt_n_threads(work_size):
    """The reference's own opt_n_threads() (cuda_utils.h), i.e. the FPS launcher's block size for a cloud of `work_size` points; host only."""
    return lib().g4d_ref_opt_n_threads(int(work_size))


def _dims(**kw):
    for k, v in kw.items():
        if int(v) <= 0:
            raise ValueError(f"{k} = {v}: the reference build is never given an empty grid")


def _t(t, dtype, numel, name):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} device tensor")
    if t.numel() != numel:
        raise ValueError(f"{name} has {t.numel()} elements, the dimensions say {numel}")
    return t.data_ptr()


def _f(t, numel, name):
    import torch
    return _t(t, torch.float32, numel, name)


def _i(t, numel, name):
    import torch
    return _t(t, torch.int32, numel, name)


def _idx(t, numel, bound, name):
    p = _i(t, numel, name)
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= bound:
        raise ValueError(f"{name} has entries in [{lo}, {hi}], outside [0, {bound}): the reference's kernels do not check")
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def ball_query_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx):
    _dims(b=b, n=n, m=m, nsample=nsample)
    lib().g4d_ref_ball_query(b, n, m, float(radius), nsample, _f(new_xyz, b * m * 3, "new_xyz"), _f(xyz, b * n * 3, "xyz"),
                             _i(idx, b * m * nsample, "idx"), _stream())
    return 1


def group_points_wrapper(b, c, n, npoints, nsample, points, idx, out):
    _dims(b=b, c=c, n=n, npoints=npoints, nsample=nsample)
    lib().g4d_ref_group(b, c, n, npoints, nsample, _f(points, b * c * n, "points"), _idx(idx, b * npoints * nsample, n, "idx"),
                        _f(out, b * c * npoints * nsample, "out"), _stream())
    return 1


def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out, idx, grad_points):
    _dims(b=b, c=c, n=n, npoints=npoints, nsample=nsample)
    lib().g4d_ref_group_grad(b, c, n, npoints, nsample, _f(grad_out, b * c * npoints * nsample, "grad_out"),
                             _idx(idx, b * npoints * nsample, n, "idx"), _f(grad_points, b * c * n, "grad_points"), _stream())
    return 1


def gather_points_wrapper(b, c, n, npoints, points, idx, out):
    _dims(b=b, c=c, n=n, npoints=npoints)
    lib().g4d_ref_gather(b, c, n, npoints, _f(points, b * c * n, "points"), _idx(idx, b * npoints, n, "idx"),
                         _f(out, b * c * npoints, "out"), _stream())
    return 1


def gather_points_grad_wrapper(b, c, n, npoints, grad_out, idx, grad_points):
    _dims(b=b, c=c, n=n, npoints=npoints)
    lib().g4d_ref_gather_grad(b, c, n, npoints, _f(grad_out, b * c * npoints, "grad_out"), _idx(idx, b * npoints, n, "idx"),
                              _f(grad_points, b * c * n, "grad_points"), _stream())
    return 1


def furthest_point_sampling_wrapper(b, n, m, points, temp, idx):
    _dims(b=b, n=n, m=m)
    lib().g4d_ref_fps(b, n, m, _f(points, b * n * 3, "points"), _f(temp, b * n, "temp"), _i(idx, b * m, "idx"), _stream())
    return 1


def three_nn_wrapper(b, n, m, unknown, known, dist2, idx):
    _dims(b=b, n=n, m=m)
    lib().g4d_ref_three_nn(b, n, m, _f(unknown, b * n * 3, "unknown"), _f(known, b * m * 3, "known"), _f(dist2, b * n * 3, "dist2"),
                           _i(idx, b * n * 3, "idx"), _stream())


def three_interpolate_wrapper(b, c, m, n, points, idx, weight, out):
    _dims(b=b, c=c, m=m, n=n)
    lib().g4d_ref_three_interp(b, c, m, n, _f(points, b * c * m, "points"), _idx(idx, b * n * 3, m, "idx"), _f(weight, b * n * 3, "weight"),
                               _f(out, b * c * n, "out"), _stream())


def three_interpolate_grad_wrapper(b, c, n, m, grad_out, idx, weight, grad_points):
    _dims(b=b, c=c, n=n, m=m)
    lib().g4d_ref_three_interp_grad(b, c, n, m, _f(grad_out, b * c * n, "grad_out"), _idx(idx, b * n * 3, m, "idx"),
                                    _f(weight, b * n * 3, "weight"), _f(grad_points, b * c * m, "grad_points"), _stream())
