"""Garment post-processing on HIP: what utils/post_processing.py:299-319 does to the last refinement round before the reference shows a mesh --
100 alternating (Taubin) Laplacian smoothing steps, then up to five rounds of `remove_interpenetration_fast` (:179-228): nearest point on the
body SURFACE for every garment vertex, vertices behind the surface get a target `eps` in front of it, and one sparse least-squares problem
trades those targets against the mesh Laplacian.  The reference runs this one frame at a time on the CPU (psbody's AABB tree + scipy's
spsolve); here all frames run at once on csrc/postprocess.hip and csrc/mesh_nearest.hip.

psbody.mesh is third-party code that is not available to this project: include/g4d.h states the definitions these kernels implement
(TriNormals / VertNormals / AabbTree.nearest as documented, post_processing.py as written); tests/postprocess_twin.py restates them in float64.

Everything is fp32 on the current torch stream; no atomics and no host round trip inside the calls, so a caller may capture them in a hipGraph
-- AFTER one eager call, which builds the per-topology tables (face order, vertex -> face CSR, Laplacian) on the host and caches them by the
identity of the `faces` / `adj_old` objects.  Outside the kernels' domain (mesh_tables.MAX_VG, MAX_ROW entries per row of the operators) the calls raise
NotImplementedError: there is no fallback."""
import collections

import numpy as np
import torch

from . import _cache
from . import _lib
from . import mesh_tables
from . import tuning
from .garment_lbs import _smoothing_csr
from .mesh_tables import MAX_ROW, MAX_VG      # the LDS-resident kernels' domain

Nearest = collections.namedtuple("Nearest", "point dist2 face part normal")


def _check_f32(name, t, last):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[-1] == last):
        raise TypeError(f"{name}: a float32 HIP tensor of shape (F, n, {last}) expected (no CPU fallback)")
    return t.contiguous()


# --------------------------------------------------------------------------------------------------------------------------- smoothing
def taubin_smooth(verts, adj_old, lam=0.05, mu=-0.052, iters=100):
    """verts (F,Vg,3) -> (F,Vg,3): step `it` is S <- S + c_it * ((D^-1 A - I) S), c_it = lam for even it, mu for odd it (:302-309), all steps
    in one launch (g4d_taubin_smooth_f32) -- bit-identical to `iters` alternating g4d_spmm_axpy_rows_f32 calls."""
    x = _check_f32("taubin_smooth", verts, 3)
    F_, Vg, _ = x.shape
    rowptr, colidx, vals, n, max_row = _smoothing_csr(adj_old, x.device)
    if n != Vg:
        raise ValueError(f"taubin_smooth: adj_old is {n} x {n}, the mesh has {Vg} vertices")
    if Vg > MAX_VG or max_row > MAX_ROW:
        raise NotImplementedError(f"taubin_smooth: the LDS-resident kernel takes Vg <= {MAX_VG} and <= {MAX_ROW} entries per adjacency row "
                                  f"(Vg {Vg}, longest row {max_row}); there is no fallback")
    out = torch.empty_like(x)
    _lib.call("g4d_taubin_smooth_f32", F_, Vg, 3, int(iters), float(lam), float(mu), max_row, x.data_ptr(), rowptr.data_ptr(), colidx.data_ptr(),
              vals.data_ptr(), out.data_ptr(), _lib.stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------------------------- per-topology tables
_topology_cache = {}


def _morton_order(centroids):
    """argsort of the 30-bit Morton codes of (n,3) points quantised to 10 bits per axis over their bounding box (stable: ties keep their order)."""
    c = np.asarray(centroids, dtype=np.float64)
    lo, hi = c.min(0), c.max(0)
    q = np.clip(((c - lo) / np.maximum(hi - lo, 1e-30) * 1023.0).astype(np.int64), 0, 1023)
    code = np.zeros(len(c), dtype=np.int64)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> bit) & 1) << (3 * bit + axis)
    return np.argsort(code, kind="stable")


def mesh_topology(faces, num_verts, device, template=None):
    """The constant tables of a triangle mesh, built once per `faces` object (host work + copies: call once before any hipGraph capture):
    faces in Morton order of the `template` (V,3) centroids (blocks of 64 consecutive faces stay compact under pose), the original index of
    each sorted face, and the vertex -> incident-face CSR (faces ascending per vertex: the summation order of the normals)."""
    def build():
        assert not torch.cuda.is_current_stream_capturing(), "mesh_topology: build the tables before the capture (call once eagerly)"
        f = np.ascontiguousarray((faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64))
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
            raise ValueError("mesh_topology: faces must be (nf, 3) triangles, nf >= 1")
        if f.min() < 0 or f.max() >= num_verts:
            raise ValueError(f"mesh_topology: face indices must lie in [0, {num_verts})")
        tpl = template.detach().cpu().numpy() if torch.is_tensor(template) else np.asarray(template)
        order = _morton_order(tpl.reshape(-1, 3)[f].mean(1))
        rowptr, corners = mesh_tables.vertex_corners(f, num_verts)
        dev = lambda a: mesh_tables.to_device(a, np.int32, device)
        return dict(nf=int(f.shape[0]), nv=int(num_verts), faces=dev(f), faces_sorted=dev(f[order]), face_ids=dev(order), vf_rowptr=dev(rowptr),
                    vf_fid=dev(corners // 3))

    return _cache.by_identity(_topology_cache, 16, (faces,), (int(num_verts), str(device)), build)


def vertex_normals_area(verts, topo, frame_active=None):
    """Area-weighted unit vertex normals (F,V,3): the scaled face normals (v1 - v0) x (v2 - v0) summed per vertex, normalised once; a
    zero-length sum yields the zero vector (g4d_vertex_normals_area_f32)."""
    F_, V, _ = verts.shape
    out = torch.empty_like(verts)
    _lib.call("g4d_vertex_normals_area_f32", F_, V, verts.data_ptr(), topo["faces"].data_ptr(), topo["vf_rowptr"].data_ptr(), topo["vf_fid"].data_ptr(),
              frame_active.data_ptr() if frame_active is not None else None, out.data_ptr(), _lib.stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------------------------------- nearest point
class _SearchMesh:
    """A posed mesh ready to be searched: its topology tables, per-frame vertex normals and per-frame block boxes (one pre-pass each)."""

    def __init__(self, verts, faces, template=None):
        self.verts = _check_f32("nearest_on_mesh: verts", verts, 3)
        F_, V, _ = self.verts.shape
        if template is None and (id(faces),) not in {k[0] for k in _topology_cache}:
            template = self.verts[0]     # first sight of this topology: its first frame stands in for the template (a host copy, once)
        self.topo = mesh_topology(faces, V, self.verts.device, template)
        self.normals = vertex_normals_area(self.verts, self.topo)
        self.nblocks = (self.topo["nf"] + 63) // 64
        self.boxes = torch.empty((F_, self.nblocks, 6), dtype=torch.float32, device=self.verts.device)
        _lib.call("g4d_mesh_aabb_f32", F_, V, self.topo["nf"], self.verts.data_ptr(), self.topo["faces_sorted"].data_ptr(), self.boxes.data_ptr(),
                  _lib.stream_ptr())

    def nearest(self, points, frame_active=None, visited=None):
        F_, P, _ = points.shape
        if F_ != self.verts.shape[0]:
            raise ValueError(f"nearest_on_mesh: {F_} frames of points, {self.verts.shape[0]} frames of mesh")
        dev = points.device
        out = Nearest(torch.empty((F_, P, 3), dtype=torch.float32, device=dev), torch.empty((F_, P), dtype=torch.float32, device=dev),
                      torch.empty((F_, P), dtype=torch.int32, device=dev), torch.empty((F_, P), dtype=torch.int32, device=dev),
                      torch.empty((F_, P, 3), dtype=torch.float32, device=dev))
        t = self.topo
        _lib.call("g4d_mesh_nearest_f32", F_, P, self.verts.shape[1], t["nf"], int(bool(tuning.current().nearest_cull)), points.data_ptr(),
                  self.verts.data_ptr(), t["faces_sorted"].data_ptr(), t["face_ids"].data_ptr(), self.boxes.data_ptr(), self.normals.data_ptr(),
                  frame_active.data_ptr() if frame_active is not None else None, out.point.data_ptr(), out.dist2.data_ptr(), out.face.data_ptr(),
                  out.part.data_ptr(), out.normal.data_ptr(), visited.data_ptr() if visited is not None else None, _lib.stream_ptr())
        return out


def nearest_on_mesh(points, verts, faces, template=None, visited=None):
    """points (F,P,3), verts (F,V,3), faces (nf,3) -> Nearest(point (F,P,3), dist2 (F,P), face (F,P) int32, part (F,P) int32, normal (F,P,3)).

    Per query: the triangle of smallest squared distance (ties: lowest face index), its closest point by the standard region classification
    (include/g4d.h writes the expression out), part = 0 interior, 1 / 2 / 3 edge ab / bc / ca, 4 / 5 / 6 vertex a / b / c, and the normal the
    reference derives from it (:155-175): the unit face normal, the area-weighted unit vertex normal of the corner, or the sum of an edge's
    two, divided by (norm + 1e-10).  Exact: the search skips blocks of faces by their bounding boxes only where they can neither win nor tie
    (tuning.nearest_cull / G4D_NEAREST_CULL switches the skipping off; both settings give the same bits).

    template (V,3): the pose whose face centroids order the faces (once per `faces` object); default: the first frame seen.
    visited: an int32 tensor of F * ceil(P / 64) entries that receives the number of face blocks each wave went through (measurement)."""
    pts = _check_f32("nearest_on_mesh: points", points, 3)
    return _SearchMesh(verts, faces, template).nearest(pts, visited=visited)


# --------------------------------------------------------------------------------------------------------------------- depenetration
_operator_cache = {}


def depenetration_operator(adj_old, device):
    """L = I - rownormalise(clip(adj_old, 0, 1)) (:131-142; a row without neighbours is the identity row) and its transpose as CSR tensors on
    `device`, plus the longest row of each: (rowptr, colidx, vals, rowptr_t, colidx_t, vals_t, n, max_row, max_row_t), once per adj_old object.
    Not losses.laplacian_csr's operator: that one takes the model's finished `lap_adj`, which is built without the clip."""
    def build():
        assert not torch.cuda.is_current_stream_capturing(), "depenetration_operator: build the operator before the capture (call once eagerly)"
        import scipy.sparse as sp
        A = sp.csr_matrix(adj_old).astype(np.float64)
        A.data = np.clip(A.data, 0.0, 1.0)
        A.eliminate_zeros()
        s = np.asarray(A.sum(1)).reshape(-1)
        inv = np.where(s > 0, 1.0 / np.where(s > 0, s, 1.0), 0.0)
        L = sp.csr_matrix(sp.eye(A.shape[0]) - sp.diags(inv).dot(A))
        L.sum_duplicates()
        L = mesh_tables.sorted_csr(L)
        Lt = mesh_tables.transposed(L)
        return (mesh_tables.csr_tensors(L, device) + mesh_tables.csr_tensors(Lt, device)
                + (int(L.shape[0]), mesh_tables.longest_row(L), mesh_tables.longest_row(Lt)))

    return _cache.by_identity(_operator_cache, 8, (adj_old,), str(device), build)


def remove_interpenetration(garment_v, garment_faces, body_v, body_faces, adj_old, eps=0.008, ww=2.0, rounds=5, cg_iters=32, body_template=None):
    """Up to `rounds` rounds of remove_interpenetration_fast (:179-228) on all frames at once.
    garment_v (F,Vg,3), garment_faces (nfg,3), body_v (F,V,3), body_faces (nf,3), adj_old scipy sparse (Vg,Vg).
    Returns (verts (F,Vg,3), counts (rounds,F) int32, residual (rounds,F,3)).

    One round, with (p, n) = nearest_on_mesh(v, body) and m = the garment's area-weighted unit vertex normals at v: vertex i is flagged iff
    dot(v_i - p_i, n_i) < 0; s_i = sign(dot(m_i, n_i)); d_i = (p_i - v_i) s_i; a flagged vertex gets the target p_i + eps d_i / (1e-4 + |d_i|)
    with weight ww, every other vertex its own position with weight 1; then (L^T L + diag(w^2)) x = L^T L v + w^2 t is solved -- the normal
    equations of the reference's stacked system [L; diag(w)] x = [L v; w t] -- by exactly `cg_iters` conjugate-gradient steps from x0 = v.
    counts[r, f] = vertices flagged in round r; residual[r, f] = |b - M x| / |b| per coordinate at exit, so nobody has to trust the iteration
    count: M's spectrum lies in [1, ww^2 + |L|^2] and the error contracts by ((sqrt(kappa) - 1) / (sqrt(kappa) + 1)) per step.

    A frame whose count is 0 keeps its vertices bit for bit in that round and in every later one (the reference solves once more and gets v
    back up to rounding, then stops); the decision is taken on the device -- the counts are the flag the later kernels read."""
    v0 = _check_f32("remove_interpenetration: garment_v", garment_v, 3)
    F_, Vg, _ = v0.shape
    dev = v0.device
    rowptr, colidx, vals, rowptr_t, colidx_t, vals_t, n, max_row, max_row_t = depenetration_operator(adj_old, dev)
    if n != Vg:
        raise ValueError(f"remove_interpenetration: adj_old is {n} x {n}, the garment has {Vg} vertices")
    if Vg > MAX_VG or max_row > MAX_ROW or max_row_t > MAX_ROW:
        raise NotImplementedError(f"remove_interpenetration: the LDS-resident solver takes Vg <= {MAX_VG} and <= {MAX_ROW} entries per row of L and "
                                  f"of its transpose (Vg {Vg}, longest rows {max_row} / {max_row_t}); there is no fallback")
    rounds, cg_iters = int(rounds), int(cg_iters)
    body = _SearchMesh(body_v, body_faces, body_template)      # the body does not move: its normals and boxes serve every round
    if body.verts.shape[0] != F_:
        raise ValueError(f"remove_interpenetration: {F_} garment frames, {body.verts.shape[0]} body frames")
    gtopo = mesh_topology(garment_faces, Vg, dev, v0[0] if (id(garment_faces),) not in {k[0] for k in _topology_cache} else None)
    counts = torch.zeros((rounds, F_), dtype=torch.int32, device=dev)
    residual = torch.zeros((rounds, F_, 3), dtype=torch.float32, device=dev)
    w2 = torch.empty((F_, Vg), dtype=torch.float32, device=dev)
    target = torch.empty((F_, Vg, 3), dtype=torch.float32, device=dev)
    cur, bufs = v0, [torch.empty_like(v0), torch.empty_like(v0) if rounds > 1 else None]
    st = _lib.stream_ptr()
    for r in range(rounds):
        active = counts[r - 1] if r > 0 else None
        m = vertex_normals_area(cur, gtopo, active)
        near = body.nearest(cur, active)
        _lib.call("g4d_depen_targets_f32", F_, Vg, float(eps), float(ww), cur.data_ptr(), near.point.data_ptr(), near.normal.data_ptr(), m.data_ptr(),
                  active.data_ptr() if active is not None else None, w2.data_ptr(), target.data_ptr(), counts[r].data_ptr(), st)
        nxt = bufs[r & 1]
        _lib.call("g4d_depen_solve_f32", F_, Vg, cg_iters, max_row, max_row_t, cur.data_ptr(), w2.data_ptr(), target.data_ptr(), counts[r].data_ptr(),
                  rowptr.data_ptr(), colidx.data_ptr(), vals.data_ptr(), rowptr_t.data_ptr(), colidx_t.data_ptr(), vals_t.data_ptr(), nxt.data_ptr(),
                  residual[r].data_ptr(), st)
        cur = nxt
    return (cur if rounds > 0 else v0.clone()), counts, residual


def post_process(garment_v, garment_faces, body_v, body_faces, adj_old):
    """The reference's post_process=True branch (:299-319) for all frames: remove_interpenetration(taubin_smooth(garment_v)) with its constants
    (lam 0.05, mu -0.052, 100 steps; eps 0.008, ww 2, up to 5 rounds).  Returns (verts, counts, residual) like remove_interpenetration."""
    return remove_interpenetration(taubin_smooth(garment_v, adj_old), garment_faces, body_v, body_faces, adj_old)


def post_process_output(output_dict, batch, model, body_faces=None):
    """post_process on a forward's result, all F = nbatch * T frames at once, reading what process_single_frame reads (:235-319):
    output_dict['iter_regressed_lbs_garment_v'][-1] (F,Vg,3), output_dict['garment_f_3'], batch['smpl_vertices_torch'] (nbatch,T,V,3), the body
    model's faces (`body_faces`, default: the ones the model kept from its forward) and model.adj_old."""
    g = output_dict["iter_regressed_lbs_garment_v"][-1]
    body = batch["smpl_vertices_torch"]
    body = (body if torch.is_tensor(body) else torch.from_numpy(np.asarray(body))).to(device=g.device, dtype=torch.float32)
    if body_faces is None:
        body_faces = getattr(model, "_body_faces", None)
        if body_faces is None:
            raise ValueError("post_process_output: pass body_faces (the model has not kept the body model's faces: it has not run forward yet)")
    return post_process(g.reshape(-1, g.shape[-2], 3), output_dict["garment_f_3"], body.reshape(-1, body.shape[-2], 3), body_faces, model.adj_old)
