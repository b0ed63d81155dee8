"""Host-side operator tables of the mesh kernels: a sparse matrix or a face list becomes the int32 / float32 CSR tensors a kernel walks.
The callers (gcn, garment_lbs, postprocess, losses) add their operator-specific line or two and their own cache (_cache.by_identity)."""
import numpy as np
import torch

# The domain of the LDS-resident mesh kernels (g4d_jacobi_smooth_f32, g4d_taubin_smooth_f32, g4d_depen_solve_f32): vertices, entries per row.
MAX_VG = 5104
MAX_ROW = 8


def sorted_csr(adj):
    """torch sparse (COO/CSR) or scipy sparse -> scipy CSR with sorted column indices."""
    if isinstance(adj, torch.Tensor):
        a = adj.detach().cpu()
        a = a.coalesce() if a.layout == torch.sparse_coo else a.to_sparse_coo().coalesce()
        import scipy.sparse as sp
        m = sp.coo_matrix((a.values().numpy(), (a.indices()[0].numpy(), a.indices()[1].numpy())), shape=tuple(a.shape)).tocsr()
    else:
        m = adj.tocsr()
    m.sort_indices()
    return m


def transposed(m):
    """The scipy CSR of m^T with sorted rows: row u lists the v with m[v, u] != 0 in ASCENDING v -- the documented summation order of the
    backward kernels that walk it (a defined order: their results are reproducible)."""
    mt = m.T.tocsr()
    mt.sum_duplicates()
    mt.sort_indices()
    return mt


def to_device(a, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(device)


def csr_tensors(m, device):
    """scipy CSR -> (rowptr int32, colidx int32, vals float32) on `device`."""
    return to_device(m.indptr, np.int32, device), to_device(m.indices, np.int32, device), to_device(m.data, np.float32, device)


def longest_row(m):
    return int(np.diff(m.indptr).max()) if m.shape[0] else 0


def vertex_corners(faces, num_verts):
    """The vertex -> incident-face CSR of an (nf, 3) int64 face array: (rowptr int64 (num_verts + 1), entries), the entries of vertex i
    being face * 3 + corner of every corner that names i, ascending (so the faces of a vertex ascend too)."""
    flat = faces.reshape(-1)
    rowptr = np.zeros(num_verts + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=num_verts), out=rowptr[1:])
    return rowptr, np.argsort(flat, kind="stable")
