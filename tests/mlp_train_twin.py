"""Float64 twin of the five kernels of csrc/bn_train.hip -- TEST INFRASTRUCTURE ONLY -- with the per-element error bounds an fp32 run of
the same arithmetic has to meet.  Inputs are the kernels' fp32 inputs, taken to float64 exactly; every bound below is derived from the
number of fp32 roundings on the path to the element (U = 2^-24, the unit roundoff) and is never fitted to a measured error.

Reduction depth.  The kernels cut the rows into slices of slice_rows(rows) rows; inside a slice thread (ty, tx) adds its rows ty, ty + TY,
... in order (ceil(slice / TY) additions), thread (0, tx) adds the TY partials (TY - 1), and the slice partials are added as four interleaved
chains (ceil(slices / 4)) plus three joining additions.  A sum whose longest path has D additions has |error| <= D U sum |term| to first
order; the terms' own roundings are added per kernel below.  depth() returns D for a shape.

The accuracy of the two library operations is taken from the HIP documentation of sqrtf and of fp32 division: at most 1 ulp = 2 U each.

  stats   mean:  (D + 2) U sum|y| / R                                  (D additions, the division by R: at most 1 ulp = 2 U)
          var:   the kernel's second pass subtracts its own rounded mean m^:  sum (y - m^)^2 / R = var + (mean - m^)^2  exactly, so
                 |var^ - var| <= b_mean^2 + (D + 5) U (var + b_mean^2)        (subtraction 1, square 1 -- doubled by squaring: 3 --, / R: 2)
                 E[y^2] - mean^2 instead carries U E[y^2], which for mean 1e3 and deviation 0.1 is 6 times the variance itself.
  act     invstd = 1 / sqrt(var + eps): U + 2 U + 2 U = 5 U;  xhat = (y - mean) invstd: + 2 U = 7 U;  z = fma(xhat, gamma, beta):
          |z^ - z| <= 7 U |gamma xhat| + U |z| =: b_z.   With the ReLU an entry with |z| <= b_z is FLAGGED: fp32 may clamp it where float64
          does not (or the reverse); its output still lies within 2 b_z, its gradient may be another element's.
  reduce  G = dOut where z > 0.  dbeta: (D + 1) U sum|G|;  dgamma: (D + 9) U sum|G xhat|  (xhat 7 U, the product 1, slack 1);  plus, for
          every flagged entry of the column, |dOut| resp. |dOut xhat| (the entry may be counted or not).
  grad    dY = a (G - mb - xhat mg), a = gamma invstd (6 U), mb = dbeta / R, mg = dgamma / R (2 U each), xhat mg (7 + 2 + 1 = 10 U), two
          subtractions and the product with a (3 U):  |dY^ - dY| <= 19 U |a| (|G| + |mb| + |xhat mg|).  Flagged entries are not compared.
          batch_stats = 0:  dY = a G,  7 U |a G|.
  pool    the first row of a group attaining the column's maximum: exact, no bound.
"""
import numpy as np

U = 2.0 ** -24
SLICE_MIN, MAX_SLICES = 64, 1024     # csrc/bn_train.hip: kBnSliceMin, kBnMaxSlices (checked against g4d_bn_slice_rows by the tests)


def slice_rows(rows):
    sr = (rows + MAX_SLICES - 1) // MAX_SLICES
    sr = (sr + 7) // 8 * 8
    return max(sr, SLICE_MIN)


def slices(rows):
    return 0 if rows <= 0 else (rows + slice_rows(rows) - 1) // slice_rows(rows)


def depth(rows, c):
    groups = c // 4 if c % 4 == 0 else c
    tx = 1
    while tx < groups and tx < 256:
        tx *= 2
    ty = 256 // tx
    sr = slice_rows(rows)
    return -(-sr // ty) + (ty - 1) + -(-slices(rows) // 4) + 3


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def stats(Y):
    """Y (rows, c) fp32 -> mean, var (biased), b_mean, b_var, all (c,) float64."""
    y = _f64(Y)
    R, c = y.shape
    D = depth(R, c)
    mean = y.mean(axis=0)
    var = ((y - mean) ** 2).mean(axis=0)
    b_mean = (D + 2) * U * np.abs(y).sum(axis=0) / R
    b_var = b_mean ** 2 + (D + 5) * U * (var + b_mean ** 2)
    return mean, var, b_mean, b_var


def _xhat(Y, mean, var, eps):
    return (_f64(Y) - _f64(mean)) / np.sqrt(_f64(var) + float(np.float32(eps)))


def act(Y, mean, var, eps, gamma, beta, relu):
    """-> out, z, xhat, b_z, flagged (all (rows, c)); gamma / beta None: 1 / 0."""
    xh = _xhat(Y, mean, var, eps)
    g = 1.0 if gamma is None else _f64(gamma)
    b = 0.0 if beta is None else _f64(beta)
    z = xh * g + b
    b_z = U * (7 * np.abs(g * xh) + np.abs(z))
    flagged = (np.abs(z) <= b_z) if relu else np.zeros(z.shape, bool)
    out = np.where(z > 0, z, 0.0) if relu else z
    return out, z, xh, b_z, flagged


def grad_reduce(dOut, Y, mean, var, eps, gamma, beta, relu):
    """-> dgamma, dbeta, b_dgamma, b_dbeta (c,), flagged (rows, c)."""
    _, z, xh, _, flagged = act(Y, mean, var, eps, gamma, beta, relu)
    d = _f64(dOut)
    R, c = d.shape
    D = depth(R, c)
    G = np.where(z > 0, d, 0.0) if relu else d
    dbeta, dgamma = G.sum(axis=0), (G * xh).sum(axis=0)
    fl = np.where(flagged, np.abs(d), 0.0)
    b_dbeta = (D + 1) * U * np.abs(G).sum(axis=0) + fl.sum(axis=0)
    b_dgamma = (D + 9) * U * np.abs(G * xh).sum(axis=0) + (fl * np.abs(xh)).sum(axis=0)
    return dgamma, dbeta, b_dgamma, b_dbeta, flagged


def grad(dOut, Y, mean, var, eps, gamma, beta, relu, batch_stats, dgamma=None, dbeta=None):
    """-> dY, b_dY, flagged (rows, c); dgamma / dbeta: the (fp32) column sums the kernel is given."""
    _, z, xh, _, flagged = act(Y, mean, var, eps, gamma, beta, relu)
    d = _f64(dOut)
    R = d.shape[0]
    G = np.where(z > 0, d, 0.0) if relu else d
    a = (1.0 if gamma is None else _f64(gamma)) / np.sqrt(_f64(var) + float(np.float32(eps)))
    if not batch_stats:
        dY = a * G
        return dY, 7 * U * np.abs(dY), flagged
    mb, mg = _f64(dbeta) / R, _f64(dgamma) / R
    dY = a * (G - mb - xh * mg)
    b = 19 * U * np.abs(a) * (np.abs(G) + np.abs(mb) + np.abs(xh * mg))
    return dY, b, flagged


def pool_max_grad(X, dP, S):
    """X (groups * S, c), dP (groups, c) -> dX (groups * S, c): dP at the first maximal row of each group, 0 elsewhere (exact)."""
    X, dP = np.asarray(X), np.asarray(dP)
    groups, c = dP.shape
    x3 = X.reshape(groups, S, c)
    arg = x3.argmax(axis=1)                         # numpy: the first occurrence
    dX = np.zeros_like(x3)
    gi, ci = np.meshgrid(np.arange(groups), np.arange(c), indexing="ij")
    dX[gi, arg, ci] = dP
    return dX.reshape(groups * S, c)


def block_step(X, W, bias, gamma, beta, eps, relu, dOut, train, running=None, pool_S=0):
    """One conv + BN + act (+ row max-pool) block, forward and backward, from the twin's pieces in float64: the composition mlp_train.py
    launches.  train: batch statistics; else `running` = (mean, var).  dOut is the cotangent of the (pooled) output.
    -> dict(out, mean, var_biased, var_unbiased, dX, dW, dbias, dgamma, dbeta)."""
    X, W = _f64(X), _f64(W)
    Yv = X @ W.T + (0.0 if bias is None else _f64(bias))
    R = Yv.shape[0]
    if train:
        mean, var = Yv.mean(axis=0), ((Yv - Yv.mean(axis=0)) ** 2).mean(axis=0)
    else:
        mean, var = _f64(running[0]), _f64(running[1])
    xh = (Yv - mean) / np.sqrt(var + float(np.float32(eps)))
    g = 1.0 if gamma is None else _f64(gamma)
    z = xh * g + (0.0 if beta is None else _f64(beta))
    out = np.where(z > 0, z, 0.0) if relu else z
    res = dict(mean=mean, var_biased=var, var_unbiased=var * R / max(R - 1, 1))
    d = _f64(dOut)
    if pool_S:
        res["out"] = out.reshape(-1, pool_S, out.shape[1]).max(axis=1)
        d = pool_max_grad(out, d, pool_S)
    else:
        res["out"] = out
    G = np.where(z > 0, d, 0.0) if relu else d
    res["dbeta"], res["dgamma"] = G.sum(axis=0), (G * xh).sum(axis=0)
    a = g / np.sqrt(var + float(np.float32(eps)))
    dY = a * (G - res["dbeta"] / R - xh * res["dgamma"] / R) if train else a * G
    res["dW"], res["dbias"], res["dX"] = dY.T @ X, dY.sum(axis=0), dY @ W
    return res
