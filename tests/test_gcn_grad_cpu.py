"""The GCN gradient route's host side (no GPU): the opt-in switch, the builder of the transposed CSR, and the fixture
tests/golden/gcn_grad.npz (the reference's own autograd, tests/golden/make_golden_gcn_grad.py) against this suite's float64 twin."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_grad_twin as TW
from garment4d_amd import gcn as G
from garment4d_amd import tuning

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_switch_is_off_by_default_and_read_from_the_environment(monkeypatch):
    assert tuning.Tuning().gcn_autograd is False
    monkeypatch.delenv("G4D_GCN_AUTOGRAD", raising=False)
    assert tuning.from_environment().gcn_autograd is False
    monkeypatch.setenv("G4D_GCN_AUTOGRAD", "1")
    assert tuning.from_environment().gcn_autograd is True
    monkeypatch.setenv("G4D_GCN_AUTOGRAD", "0")
    assert tuning.from_environment().gcn_autograd is False
    t = tuning.current().replace(gcn_autograd=True)
    assert t.gcn_autograd is True
    with tuning.use(t):
        assert tuning.current().gcn_autograd is True
    assert tuning.current().gcn_autograd is tuning.DEFAULT.gcn_autograd


def _check_transposed(adj, dense):
    rowptr, colidx, vals, n = G._to_csr_t(adj, torch.device("cpu"))
    want = sp.csr_matrix(dense).T.tocsr()
    want.sum_duplicates(); want.sort_indices()
    assert n == dense.shape[1] and rowptr.dtype == torch.int32 and colidx.dtype == torch.int32 and vals.dtype == torch.float32
    assert np.array_equal(rowptr.numpy(), want.indptr) and np.array_equal(colidx.numpy(), want.indices)
    assert np.array_equal(vals.numpy(), want.data.astype(np.float32))
    for u in range(n):   # ascending column indices inside every row: the summation order of dS
        c = colidx.numpy()[rowptr[u]:rowptr[u + 1]]
        assert np.all(np.diff(c) > 0)
    back = sp.csr_matrix((vals.numpy(), colidx.numpy(), rowptr.numpy()), shape=(n, dense.shape[0])).toarray()
    assert np.array_equal(back, dense.T.astype(np.float32))


def test_transposed_csr_of_the_fixture_mesh():
    _, g = TW.load()
    A = TW.dense_adjacency(g).astype(np.float32)
    m = sp.csr_matrix((g["adj_val"], (g["adj_row"], g["adj_col"])), shape=(64, 64))
    _check_transposed(m, A)
    _check_transposed(G.sparse_mx_to_torch_sparse_tensor(m), A)
    assert not np.array_equal(A, A.T)   # row-normalised: the transpose is a different matrix, a builder returning A itself would be caught


def test_transposed_csr_empty_row_empty_column_duplicates_and_cache():
    dense = np.zeros((6, 6), dtype=np.float32)
    dense[0, 1], dense[0, 4], dense[1, 0], dense[3, 1], dense[4, 4], dense[5, 0], dense[5, 1] = 0.5, 0.25, 1.0, 2.0, 0.125, 3.0, 0.75
    assert not dense[2].any() and not dense[:, 2].any() and not dense[:, 3].any() and not dense[:, 5].any()   # empty row 2; empty columns 2, 3, 5
    r, c = np.nonzero(dense)
    _check_transposed(sp.coo_matrix((dense[r, c], (r, c)), shape=(6, 6)).tocsr(), dense)
    # duplicate COO entries are summed: (0, 1) given as 0.25 + 0.25, (5, 0) as 1 + 2
    rr = np.concatenate([r, [0, 5]]); cc = np.concatenate([c, [1, 0]])
    vv = dense[r, c].copy(); vv[(r == 0) & (c == 1)] = 0.25; vv[(r == 5) & (c == 0)] = 1.0
    vv = np.concatenate([vv, [0.25, 2.0]]).astype(np.float32)
    t = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([rr, cc]).astype(np.int64)), torch.from_numpy(vv), (6, 6))
    _check_transposed(t, dense)
    first = G._to_csr_t(t, torch.device("cpu"))
    again = G._to_csr_t(t, torch.device("cpu"))
    assert all(a is b for a, b in zip(first[:3], again[:3]))


def test_fixture_has_no_relu_coin_toss():
    g, _ = TW.load()
    assert float(g["stack_min_preact"]) >= 2e-5


def test_float64_twin_reproduces_the_single_layer_gradients():
    """Dense float64 numpy against the float64 gradients torch's autograd gave for the reference's layer: 1e-12 relative (to the tensor's max)."""
    g, o = TW.load()
    A = TW.dense_adjacency(o)
    for name, ismlp in (("l3d", False), ("l2d", False), ("mlp", True), ("nb", False)):
        dx, dW, db = TW.layer_backward(g[f"{name}_x"], g[f"{name}_W"], A, g[f"{name}_dy"].astype(np.float64), ismlp=ismlp)
        for k, got in (("dx", dx), ("dW", dW), ("db", db)):
            if f"{name}_{k}64" not in g.files:
                assert name == "nb" and k == "db"
                continue
            ref = g[f"{name}_{k}64"]
            assert ref.dtype == np.float64 and got.shape == ref.shape
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (name, k)
            # and the stored fp32 gradient is that float64 one up to fp32 rounding of its sums
            assert np.abs(g[f"{name}_{k}"] - ref).max() <= 1e-5 * np.abs(ref).max(), (name, k)


def test_float64_twin_reproduces_the_stack_error_figures():
    """The stack's float64 gradients are not stored; the twin recomputes them and its distance to the stored fp32 gradients must be the
    stored e_ref (max |ref32 - ref64|) to 1e-9 relative, its maximum the stored max |ref64|, its smallest hidden |pre-activation| the
    stored one: the twin IS the reference's float64 run up to float64 rounding.  (1e-9 of e_ref is ~1e-16 of the gradients themselves, the
    size of ONE float64 rounding: the twin runs in extended precision here so that only the reference run's own float64 rounding is left;
    in float64 the twin's rounding adds to it and db2 sits at 3.8e-9.)"""
    g, o = TW.load()
    A = TW.dense_adjacency(o)
    grads, pres = TW.stack_grads(g["stack_x"], [g[f"stack_W{i}"] for i in range(4)], [g[f"stack_b{i}"] for i in range(4)], A, g["stack_dy"],
                                  dt=np.longdouble)
    assert set(grads) == {"dx"} | {f"dW{i}" for i in range(4)} | {f"db{i}" for i in range(4)}
    for k, ref64 in grads.items():
        e = float(np.abs(g[f"stack_{k}"].astype(np.longdouble) - ref64).max())
        assert abs(e - float(g[f"stack_eref_{k}"])) <= 1e-9 * float(g[f"stack_eref_{k}"]), (k, e, float(g[f"stack_eref_{k}"]))
        assert abs(float(np.abs(ref64).max()) - float(g[f"stack_max64_{k}"])) <= 1e-12 * float(g[f"stack_max64_{k}"]), k
    mn = min(float(np.abs(p).min()) for p in pres)
    assert abs(mn - float(g["stack_min_preact"])) <= 1e-9 * mn and mn >= 2e-5


@pytest.mark.skipif(not os.environ.get("G4D_REFERENCE_DIR"), reason="needs a checkout of the reference (G4D_REFERENCE_DIR)")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    env = dict(os.environ, G4D_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_gcn_grad.py")], env=env, cwd=ROOT)
    new, (old, _) = np.load(os.path.join(str(tmp_path), "gcn_grad.npz")), TW.load()
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k
