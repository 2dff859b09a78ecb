"""Reconstruction metrics on the device: what code/evaluation/eval_rec.py computes with scipy's cKDTree, open3d's ICP and
trimesh's surface sampling.

* ``NNIndex`` / ``nearest``: exact fp32 nearest neighbours (C ABI Section 8, csrc/mesh_eval.hip), ties to the lowest index.
  ``NNIndex.knn`` / ``nearest_k``: the k nearest under the total order (d2, index) (C ABI Section 28).
* ``sample_surface``: area-weighted surface samples from the engine's Philox stream (trimesh.sample.sample_surface).
* ``icp_point_to_point``: open3d's registration_icp with TransformationEstimationPointToPoint and default criteria;
  ``with_scaling`` estimates a scale as well (CloudCompare's -ICP -ADJUST_SCALE, eval_rec.py:274).
* ``mesh_metrics``: calc_3d_metric + calc_normal_consistency (eval_rec.py:143-166, 207-236) from one ICP and one sample set,
  optionally after the similarity of the trajectory evaluation and the removal of stray components (eval_rec.py:259-272,
  nicer_slam_amd/mesh_clean.py).
* ``TriIndex`` / ``closest_point`` / ``distance_p2m``: the exact closest point of a triangle mesh for each query point, in float64
  (C ABI Section 14, csrc/mesh_closest.hip; trimesh.proximity.closest_point of eval_rec.py:120-129).
  ``TriIndex.signed_query`` and ``query(max_dist=)``: the signed and the range-limited form (C ABI Section 15, csrc/mesh_sdf.hip,
  DESIGN 4n; nicer_slam_amd/mesh_sdf.py builds SDF grids and field metrics on them).  ``TriIndex.raycast``: the exact first hit of
  rays against the mesh (C ABI Section 17, csrc/mesh_raycast.hip; nicer_slam_amd/mesh_raycast.py renders depth with it).
* ``mesh_metrics(..., surface="mesh")``: the same metrics from the distance of each sample to the other mesh's SURFACE, which a
  perfect reconstruction scores 0 on; the default ``surface="samples"`` is the reference's sample-to-sample form.
* ``mesh_metrics(..., icp="plane" | "surface")``: the alignment by point-to-plane ICP against the ground truth's vertices and normals
  or against its surface (nicer_slam_amd/mesh_register.py); the default ``icp="point"`` is the reference's.
* ``python -m nicer_slam_amd.mesh_eval REC.ply GT.ply [--sim3 T.npy] [--clean largest] [--adjust-scale] [--surface mesh]
  [--icp point|plane|surface]``: the reference's printout.

Reductions over the distance arrays (means, counts, ICP's centroids and cross-covariance) run in torch float64: they are small
and deterministic.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import math

import numpy as np
import torch

from ._native import KNN_MAX_K, RAY_ANY_HIT, RAY_BRUTE, RAY_CULL_BACK, RAY_CULL_FRONT, check, lib
from .mesh_args import MAX_FACES, checked_faces, checked_points, cuda_verts_faces, max_d2 as _max_d2, need_gpu, stream, workspace
from .ply import read_ply

F_THRESHOLDS = (0.010, 0.015, 0.020)       # np.linspace(1/1000, 1, 1000)[[9, 14, 19]] of eval_pointcloud
COMPLETION_RATIO_THRESHOLD = 0.05          # completion_ratio's dist_th (eval_rec.py:168)


class NNIndex:
    """Exact nearest-neighbour index over fp32 targets [n, 3] on the device, built once and queried any number of times.
    The index keeps its own copy of the targets (sorted by grid cell); the tensor passed in may change afterwards."""

    @torch.no_grad()
    def __init__(self, targets):
        t = checked_points(targets, "NNIndex")
        self.n = t.shape[0]
        if self.n == 0:
            raise ValueError("NNIndex: no targets")
        self.device = t.device
        self.buf = workspace(lib.nsa_nn_workspace(self.n), t.device)
        check(lib.nsa_nn_build(t.data_ptr(), self.n, self.buf.data_ptr(), stream(t.device)))

    @torch.no_grad()
    def query(self, queries, max_dist=math.inf):
        """(dist [m] fp32, idx [m] int64): the nearest target of each query, ties to the lowest index.  With a finite
        ``max_dist`` only targets with d2 < fp32(max_dist^2) count (open3d's hybrid search); none gives (+inf, -1).
        A non-finite query gives (NaN, -1)."""
        q = checked_points(queries, "NNIndex.query")
        if q.device != self.device:
            raise ValueError("NNIndex.query: queries on another device than the index")
        if not max_dist > 0:
            raise ValueError("NNIndex.query: max_dist must be > 0")
        m = q.shape[0]
        idx = torch.empty(m, dtype=torch.int32, device=q.device)
        dist = torch.empty(m, dtype=torch.float32, device=q.device)
        if m:
            check(lib.nsa_nn_query(self.buf.data_ptr(), self.n, q.data_ptr(), m, float(max_dist), idx.data_ptr(), dist.data_ptr(),
                                   stream(q.device)))
        return dist, idx.long()

    @torch.no_grad()
    def _knn(self, q, k, max_dist, name="NNIndex.knn"):
        """nsa_nn_query_k on checked fp32 queries: (dist [m, k] fp32, idx [m, k] int32, count [m] int32 holding the uint32 counts)"""
        if q.device != self.device:
            raise ValueError(f"{name}: queries on another device than the index")
        if not (isinstance(k, int) and 1 <= k <= KNN_MAX_K):
            raise ValueError(f"{name}: k must be an integer in [1, {KNN_MAX_K}], got {k!r}")
        if not max_dist > 0:
            raise ValueError(f"{name}: max_dist must be > 0")
        m = q.shape[0]
        idx = torch.empty(m, k, dtype=torch.int32, device=q.device)
        dist = torch.empty(m, k, dtype=torch.float32, device=q.device)
        count = torch.empty(m, dtype=torch.int32, device=q.device)
        if m:
            check(lib.nsa_nn_query_k(self.buf.data_ptr(), self.n, q.data_ptr(), m, k, float(max_dist), idx.data_ptr(), dist.data_ptr(),
                                     count.data_ptr(), stream(q.device)))
        return dist, idx, count

    def knn(self, queries, k, max_dist=math.inf):
        """(dist [m, k] fp32, idx [m, k] int64, count [m] int64): the ``k`` (1 .. 64) nearest targets of each query under the total
        order (d2, target index), in that order (C ABI Section 28): exact ties go to the lower index, at the k-th place too.  With a
        finite ``max_dist`` only targets with d2 < fp32(max_dist^2) count.  ``count`` is the number found; the slots behind it hold
        (+inf, -1).  A non-finite query gives count 0 and (NaN, -1).  ``knn(q, 1)`` is ``query(q)`` with a column axis."""
        dist, idx, count = self._knn(checked_points(queries, "NNIndex.knn"), k, max_dist)
        return dist, idx.long(), count.long()

    def grid(self):
        """(lo [3], cell size [3], cells per axis [3], per-cell point counts [Rx, Ry, Rz]) of the built grid (host copies;
        a synchronisation -- for measurements, not for the query path)."""
        head = self.buf[:64].cpu().numpy()
        lo, h = head[:12].view(np.float32), head[12:24].view(np.float32)
        R = head[36:48].view(np.uint32).astype(np.int64)
        ncells = int(R.prod())
        start = self.buf[256:256 + 4 * (ncells + 1)].view(torch.int32).long()
        counts = (start[1:] - start[:-1]).view(*R.tolist())
        return lo.copy(), h.copy(), R, counts


@torch.no_grad()
def nearest(queries, targets, max_dist=math.inf):
    """(dist, idx) of the nearest target of each query (``NNIndex(targets).query(queries, max_dist)``)."""
    return NNIndex(targets).query(queries, max_dist)


@torch.no_grad()
def nearest_k(queries, targets, k, max_dist=math.inf):
    """(dist, idx, count) of the ``k`` nearest targets of each query (``NNIndex(targets).knn(queries, k, max_dist)``)."""
    return NNIndex(targets).knn(queries, k, max_dist)


@torch.no_grad()
def sample_surface(verts, faces, n, seed=0):
    """(points [n, 3] fp32, face_idx [n] int64): ``n`` area-weighted samples of the triangle mesh, from Philox4x32-10 with
    key = seed and counter = sample index (trimesh.sample.sample_surface, restated in include/nicer_slam_amd.h Section 8).
    Raises ValueError for a mesh without faces or with zero (or non-finite) total area."""
    v = checked_points(verts, "sample_surface")
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError("sample_surface: faces must be a CUDA tensor [F, 3]")
    f = faces.to(torch.int32).contiguous()
    V, F = v.shape[0], f.shape[0]
    if V == 0 or F == 0:
        raise ValueError("sample_surface: empty mesh")
    if F >= 1 << 31 or n >= 1 << 31 or n < 0:
        raise ValueError("sample_surface: count out of range")
    if int(f.min()) < 0 or int(f.max()) >= V:
        raise ValueError("sample_surface: face index out of range")
    ws = workspace(lib.nsa_surface_sample_workspace(F), v.device)
    pts = torch.empty(n, 3, device=v.device)
    fidx = torch.empty(n, dtype=torch.int32, device=v.device)
    total = torch.empty(1, dtype=torch.float64, device=v.device)
    check(lib.nsa_surface_sample(v.data_ptr(), V, f.data_ptr(), F, n, int(seed) & (2 ** 64 - 1), ws.data_ptr(),
                                 pts.data_ptr() if n else None, fidx.data_ptr() if n else None, total.data_ptr(),
                                 stream(v.device)))
    a = float(total)
    if not (a > 0 and math.isfinite(a)):
        raise ValueError(f"sample_surface: total area {a} (zero-area or non-finite mesh)")
    return pts, fidx.long()


def welded_faces(verts, faces):
    """``faces`` [F, 3] int32 with every vertex named by the rank of its fp32 coordinates among the distinct ones (-0 = +0), the
    naming of ``TriIndex.adjacency(weld=True)`` and ``mesh_topology.topology(weld=True)``; a face with an index outside [0, V) is
    kept as it is.  ``torch.unique`` of the coordinates, wherever ``verts`` lives."""
    # + 0.0: -0 becomes +0.  A non-finite vertex is named as (0, 0, 0): NaN rows break the sort inside torch.unique,
    # and what they share a name with does not matter, as no face with such a vertex contributes
    finite = torch.isfinite(verts).all(1, keepdim=True)
    _, inverse = torch.unique(torch.where(finite, verts + 0.0, torch.zeros_like(verts)), dim=0, return_inverse=True)
    ok = ((faces >= 0) & (faces < verts.shape[0])).all(1, keepdim=True)
    safe = torch.where(ok, faces, torch.zeros_like(faces)).long()
    return torch.where(ok, inverse[safe].to(torch.int32), faces).contiguous()


class TriIndex:
    """Exact closest-point index over a triangle mesh (fp32 verts [V, 3], integer faces [F, 3]) on the device, built once and
    queried any number of times (include/nicer_slam_amd.h Section 14).  The index refers to the mesh by face number, so it keeps
    its own fp32 / int32 copies of both arrays; the tensors passed in may change afterwards.  Faces with an index outside
    [0, V), a non-finite vertex or zero area are skipped and counted in ``skipped`` (in that order)."""

    @torch.no_grad()
    def __init__(self, verts, faces):
        v = checked_points(verts, "TriIndex")
        f = checked_faces(faces, "TriIndex", max_faces=MAX_FACES, dtypes=None, require_cuda=True).to(torch.int32).contiguous()
        if v.device != f.device:
            raise ValueError("TriIndex: verts and faces on different devices")
        if v.shape[0] == 0 or f.shape[0] == 0:
            raise ValueError("TriIndex: empty mesh")
        self.verts = v.clone() if v.data_ptr() == verts.data_ptr() else v
        self.faces = f.clone() if f.data_ptr() == faces.data_ptr() else f
        self.V, self.F = v.shape[0], f.shape[0]
        self.device = v.device
        self.buf = workspace(lib.nsa_tri_workspace(self.F), v.device)
        self._totals = torch.zeros(3, dtype=torch.int32, device=v.device)
        check(lib.nsa_tri_build(self.verts.data_ptr(), self.V, self.faces.data_ptr(), self.F, self.buf.data_ptr(),
                                self._totals.data_ptr(), stream(v.device)))
        self._adjacency = {}                       # weld setting -> (adjacency faces, adjacency buffer), built on first use
        self._winding = None                       # (tree buffer, info) of Section 16, built on first use
        self._ray = None                           # (tree buffer, info) of Section 17, built on first use
        self._topology = {}                        # weld setting -> report of Section 18, computed on first use
        self._orientation = {}                     # weld setting -> result of Section 20, computed on first use

    @property
    def skipped(self):
        """(bad index, non-finite vertex, zero area) face counts (a host copy: a synchronisation)"""
        return tuple(int(x) for x in self._totals.cpu())

    @torch.no_grad()
    def query(self, points, counts=False, squared=False, max_dist=None):
        """(dist [m] float64, face [m] int64, closest [m, 3] fp32): the closest point of the mesh for each query, the distance
        to it (the square root, in torch float64, of the kernel's float64 d2) and the face it lies on, ties to the lowest face
        index.  A non-finite query gives (NaN, -1, NaN); a mesh without a usable face (+inf, -1, NaN).  ``squared=True`` returns the
        kernel's d2 itself in place of dist; ``counts=True`` appends the number of faces fully evaluated per query [m] int64 (a
        measurement of the index).  ``max_dist`` (None: unbounded, the path of every call without it): only a closest point with
        d2 <= max_dist^2 counts, any other query gives (+inf, -1, NaN), and the walk stops once nothing within max_dist is left
        (header Section 15); ``counts=True`` then appends the cells visited per query as well."""
        q = checked_points(points, "TriIndex.query")
        if q.device != self.device:
            raise ValueError("TriIndex.query: points on another device than the index")
        m = q.shape[0]
        face = torch.empty(m, dtype=torch.int32, device=q.device)
        d2 = torch.empty(m, dtype=torch.float64, device=q.device)
        closest = torch.empty(m, 3, dtype=torch.float32, device=q.device)
        n_eval = torch.zeros(m, dtype=torch.int32, device=q.device) if counts else None
        if max_dist is not None:
            n_cells = torch.zeros(m, dtype=torch.int32, device=q.device) if counts else None
            if m:
                check(lib.nsa_tri_query_bounded(self.buf.data_ptr(), self.verts.data_ptr(), self.V, self.faces.data_ptr(), self.F,
                                                q.data_ptr(), m, _max_d2(max_dist, "TriIndex.query"), face.data_ptr(), d2.data_ptr(),
                                                closest.data_ptr(), n_eval.data_ptr() if counts else None,
                                                n_cells.data_ptr() if counts else None,
                                                stream(q.device)))
            else:
                _max_d2(max_dist, "TriIndex.query")
            out = (d2 if squared else torch.sqrt(d2), face.long(), closest)
            return out + (n_eval.long(), n_cells.long()) if counts else out
        if m:
            check(lib.nsa_tri_query_counted(self.buf.data_ptr(), self.verts.data_ptr(), self.V, self.faces.data_ptr(), self.F,
                                            q.data_ptr(), m, face.data_ptr(), d2.data_ptr(), closest.data_ptr(),
                                            n_eval.data_ptr() if counts else None,
                                            stream(q.device)))
        out = (d2 if squared else torch.sqrt(d2), face.long(), closest)
        return out + (n_eval.long(),) if counts else out

    def adjacency(self, weld=True):
        """(adjacency faces [F, 3] int32, adjacency buffer) of header Section 15, built on first use and kept, once per ``weld``
        setting.  ``weld=True`` names every vertex by the rank of its fp32 coordinates among the distinct ones (-0 = +0; a face
        with a non-finite vertex is skipped whatever its names are) -- ``torch.unique`` of the coordinates on the device
        -- so that a mesh whose seams repeat vertices is connected across them; ``weld=False`` takes the faces as they are."""
        weld = bool(weld)
        if weld not in self._adjacency:
            adj = welded_faces(self.verts, self.faces) if weld else self.faces
            nbytes = lib.nsa_tri_adjacency_workspace(self.V, self.F)
            if nbytes == 0:
                raise ValueError("TriIndex.adjacency: more than (2^31 - 1) / 3 faces")
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            check(lib.nsa_tri_adjacency_build(self.verts.data_ptr(), self.V, self.faces.data_ptr(), adj.data_ptr(), self.F,
                                              buf.data_ptr(), stream(self.device)))
            self._adjacency[weld] = (adj, buf)
        return self._adjacency[weld]

    def topology(self, weld=True):
        """the report of ``mesh_topology.topology`` for the index's mesh (header Section 18), computed on first use and kept, once
        per ``weld`` setting, like ``adjacency``"""
        weld = bool(weld)
        if weld not in self._topology:
            from .mesh_topology import topology              # (a cycle: mesh_topology welds and casts rays with this module)
            self._topology[weld] = topology({"verts": self.verts, "faces": self.faces}, weld=weld)
        return dict(self._topology[weld])

    def orientation(self, weld=True):
        """``mesh_topology.orientation`` for the index's mesh (header Section 20): (orient_label, orientable, flip, report), computed
        on first use and kept, once per ``weld`` setting, like ``topology``"""
        weld = bool(weld)
        if weld not in self._orientation:
            from .mesh_topology import orientation           # (the same cycle)
            self._orientation[weld] = orientation({"verts": self.verts, "faces": self.faces}, weld=weld)
        label, orientable, flip, report = self._orientation[weld]
        return label, orientable, flip, dict(report)

    @torch.no_grad()
    def signed_query(self, points, max_dist=None, flip=False, weld=True, counts=False, normals=False):
        """(signed dist [m] float64, face [m] int64, closest [m, 3] fp32, feature [m] int8): ``query``'s answer with the sign of the
        angle-weighted pseudo-normal of the closest feature (header Section 15; Baerentzen & Aanaes 2005): positive on the side the
        faces' ab x ac points to, negative on the other, ``flip`` the opposite.  Exact inside / outside for a closed manifold mesh;
        for an open one the side of the nearest surface element.  ``feature``: 0 interior, 1 / 2 / 4 vertex a / b / c, 3 / 5 / 6
        edge ab / ac / bc of ``face``, -1 without one.  A non-finite query gives (NaN, -1, NaN, -1); a query with nothing within
        ``max_dist`` (None: unbounded), or a mesh without a usable face, (+inf, -1, NaN, -1) -- -inf with ``flip``.
        ``normals=True`` appends N [m, 3] and W [m] float64; ``counts=True`` then the faces evaluated and the cells visited [m] int64."""
        q = checked_points(points, "TriIndex.signed_query")
        if q.device != self.device:
            raise ValueError("TriIndex.signed_query: points on another device than the index")
        bound = _max_d2(max_dist, "TriIndex.signed_query")
        m = q.shape[0]
        dev = q.device
        face = torch.empty(m, dtype=torch.int32, device=dev)
        d2 = torch.empty(m, dtype=torch.float64, device=dev)
        closest = torch.empty(m, 3, dtype=torch.float32, device=dev)
        feature = torch.empty(m, dtype=torch.int8, device=dev)
        sign = torch.empty(m, dtype=torch.int8, device=dev)
        N = torch.zeros(m, 3, dtype=torch.float64, device=dev) if normals else None
        W = torch.zeros(m, dtype=torch.float64, device=dev) if normals else None
        n_eval = torch.zeros(m, dtype=torch.int32, device=dev) if counts else None
        n_cells = torch.zeros(m, dtype=torch.int32, device=dev) if counts else None
        if m:
            adj, buf = self.adjacency(weld)
            check(lib.nsa_tri_signed_query_counted(self.buf.data_ptr(), buf.data_ptr(), self.verts.data_ptr(), self.V,
                                                   self.faces.data_ptr(), adj.data_ptr(), self.F, q.data_ptr(), m, bound,
                                                   1 if flip else 0, face.data_ptr(), d2.data_ptr(), closest.data_ptr(),
                                                   feature.data_ptr(), sign.data_ptr(), N.data_ptr() if normals else None,
                                                   W.data_ptr() if normals else None, n_eval.data_ptr() if counts else None,
                                                   n_cells.data_ptr() if counts else None,
                                                   stream(dev)))
        out = (sign.double() * torch.sqrt(d2), face.long(), closest, feature)
        if normals:
            out += (N, W)
        if counts:
            out += (n_eval.long(), n_cells.long())
        return out

    def _winding_tree(self):
        """(tree buffer, info [3] int32 on the device: L, node count, usable faces) of header Section 16, built on first use and kept"""
        if self._winding is None:
            buf = workspace(lib.nsa_tri_winding_workspace(self.F), self.device)
            info = torch.zeros(3, dtype=torch.int32, device=self.device)
            check(lib.nsa_tri_winding_build(self.verts.data_ptr(), self.V, self.faces.data_ptr(), self.F, buf.data_ptr(),
                                            info.data_ptr(), stream(self.device)))
            self._winding = (buf, info)
        return self._winding

    @torch.no_grad()
    def winding(self, points, beta=2.0, flip=False, counts=False):
        """[m] float64: the generalised winding number of the mesh at each point (header Section 16; Jacobson et al. 2013) -- the sum
        of the signed solid angles of the usable faces over 4 pi.  1 inside and 0 outside a closed mesh whose normals point outwards
        (``flip`` for inward ones: the negated value).  On an open mesh it is a smooth field, 1/2 across a hole's virtual closure, so
        ``w > 0.5`` is an inside / outside test that a hole does not break.  ``beta`` (>= 1): the accuracy of the hierarchical
        approximation of Barill et al. 2018 -- a tree node whose faces lie within r of its centre is used through its dipole from
        farther than beta r; 2 is theirs, ``math.inf`` the exact sum over all faces.  A non-finite point gives NaN; a mesh without a
        usable face 0.  ``counts=True`` appends the nodes accepted and the faces summed exactly per point [m] int64 (measurements).
        The tree is independent of the closest-point index and built on first use."""
        q = checked_points(points, "TriIndex.winding")
        if q.device != self.device:
            raise ValueError("TriIndex.winding: points on another device than the index")
        beta = float(beta)
        if not beta >= 1.0:
            raise ValueError(f"TriIndex.winding: beta must be >= 1, got {beta!r}")
        m = q.shape[0]
        w = torch.empty(m, dtype=torch.float64, device=q.device)
        n_acc = torch.zeros(m, dtype=torch.int32, device=q.device) if counts else None
        n_eval = torch.zeros(m, dtype=torch.int32, device=q.device) if counts else None
        if m:
            buf, _ = self._winding_tree()
            check(lib.nsa_tri_winding_query(buf.data_ptr(), self.verts.data_ptr(), self.V, self.faces.data_ptr(), self.F, q.data_ptr(),
                                            m, beta, 1 if flip else 0, w.data_ptr(), n_acc.data_ptr() if counts else None,
                                            n_eval.data_ptr() if counts else None, stream(q.device)))
        return (w, n_acc.long(), n_eval.long()) if counts else w

    def winding_layout(self):
        """dict(L, nodes, usable faces, bytes) of the winding-number tree (a host copy: a synchronisation)"""
        buf, info = self._winding_tree()
        L, nodes, usable = (int(x) for x in info.cpu())
        return {"L": L, "nodes": nodes, "usable faces": usable, "bytes": int(buf.numel())}

    def _ray_tree(self):
        """(tree buffer, info [3] int32 on the device: L, node count, usable faces) of header Section 17, built on first use and kept"""
        if self._ray is None:
            buf = workspace(lib.nsa_tri_ray_workspace(self.F), self.device)
            info = torch.zeros(3, dtype=torch.int32, device=self.device)
            check(lib.nsa_tri_ray_build(self.verts.data_ptr(), self.V, self.faces.data_ptr(), self.F, buf.data_ptr(),
                                        info.data_ptr(), stream(self.device)))
            self._ray = (buf, info)
        return self._ray

    @torch.no_grad()
    def raycast(self, origins, dirs, tmin=0.0, tmax=math.inf, any_hit=False, cull=None, counts=False, brute=False):
        """(t [m] float64, face [m] int64, bary [m, 3] float64): where each ray ``origins + t * dirs`` (CUDA tensors [m, 3]; a
        direction is not normalised, t is in units of its length) first hits the mesh within [tmin, tmax], ties to the lowest face
        index, with the barycentric coordinates of the hit for the face's three vertices (header Section 17: the watertight test of
        Woop et al. 2013 in float64 -- no ray slips between two faces that share an edge).  A miss gives (+inf, -1, NaN); a ray with a
        non-finite component or a zero direction (NaN, -1, NaN).  ``cull``: None, "back" (faces whose ab x ac points along the ray are
        not hit) or "front".  ``any_hit=True`` returns bool [m] instead -- whether anything is hit -- and stops each ray at the first
        hit found.  ``brute=True`` tests every usable face (the on-device cross-check).  ``counts=True`` appends the tree nodes
        visited and the faces tested per ray [m] int64 (measurements).  The tree is built on first use."""
        o, d = checked_points(origins, "TriIndex.raycast"), checked_points(dirs, "TriIndex.raycast")
        if o.device != self.device or d.device != self.device:
            raise ValueError("TriIndex.raycast: rays on another device than the index")
        if o.shape != d.shape:
            raise ValueError(f"TriIndex.raycast: {o.shape[0]} origins for {d.shape[0]} directions")
        tmin, tmax = float(tmin), float(tmax)
        if math.isnan(tmin) or math.isnan(tmax):
            raise ValueError("TriIndex.raycast: tmin and tmax must not be NaN")
        if cull not in (None, "back", "front"):
            raise ValueError(f"TriIndex.raycast: cull must be None, 'back' or 'front', got {cull!r}")
        flags = ((RAY_ANY_HIT if any_hit else 0) | (RAY_BRUTE if brute else 0)
                 | {None: 0, "back": RAY_CULL_BACK, "front": RAY_CULL_FRONT}[cull])
        m, dev = o.shape[0], o.device
        t = torch.empty(m, dtype=torch.float64, device=dev)
        face = torch.empty(m, dtype=torch.int32, device=dev)
        bary = None if any_hit else torch.empty(m, 3, dtype=torch.float64, device=dev)
        n_nodes = torch.zeros(m, dtype=torch.int32, device=dev) if counts else None
        n_tested = torch.zeros(m, dtype=torch.int32, device=dev) if counts else None
        if m:
            buf, _ = self._ray_tree()
            check(lib.nsa_tri_ray_cast(buf.data_ptr(), self.verts.data_ptr(), self.V, self.faces.data_ptr(), self.F, o.data_ptr(),
                                       d.data_ptr(), m, tmin, tmax, flags, t.data_ptr(), face.data_ptr(),
                                       bary.data_ptr() if bary is not None else None, n_nodes.data_ptr() if counts else None,
                                       n_tested.data_ptr() if counts else None, stream(dev)))
        out = (face >= 0,) if any_hit else (t, face.long(), bary)
        if counts:
            return out + (n_nodes.long(), n_tested.long())
        return out[0] if any_hit else out

    def self_intersections(self, kinds=("proper", "touch"), between=None, brute=False, return_report=False):
        """(pairs int64 [n, 2], code uint8 [n], flags uint8 [F]) on the index's device: the pairs of faces that meet in more than the
        positions they share, decided exactly (header Section 25; ``mesh_intersect.self_intersections`` describes the
        arguments and the report).  Walks the ray-cast tree, built on first use and kept."""
        from .mesh_intersect import _search                  # (a cycle: mesh_intersect searches a TriIndex)
        *out, report = _search(self, kinds, between, brute)
        return tuple(out) + (report,) if return_report else tuple(out)

    def ray_layout(self):
        """dict(L, nodes, usable faces, bytes) of the ray-cast tree (a host copy: a synchronisation)"""
        buf, info = self._ray_tree()
        L, nodes, usable = (int(x) for x in info.cpu())
        return {"L": L, "nodes": nodes, "usable faces": usable, "bytes": int(buf.numel())}

    def layout(self):
        """dict(cells per axis, cell size, faces in the grid, faces on the large list, faces skipped) of the built index (host
        copies; a synchronisation -- for measurements, not for the query path).  Reads csrc/mesh_closest.hip's struct Grid at the head
        of the index buffer and the start array 256 bytes in; a static_assert there holds the offsets used here."""
        head = self.buf[:64].cpu().numpy()
        h = head[12:24].view(np.float32)
        R = head[36:48].view(np.uint32).astype(np.int64)
        ncells = int(head[48:52].view(np.uint32)[0])
        st = self.buf[256 + 4 * ncells:256 + 4 * (ncells + 3)].view(torch.int32).cpu().numpy()
        return {"cells": R.tolist(), "cell size": h.tolist(), "grid faces": int(st[0]), "large faces": int(st[1] - st[0]),
                "skipped faces": int(st[2] - st[1])}


@torch.no_grad()
def closest_point(mesh, points):
    """(closest [m, 3] fp32, dist [m] float64, face [m] int64) -- the order of trimesh.proximity.closest_point -- of ``points``
    (CUDA tensor or array [m, 3]) on ``mesh`` (dict with ``verts`` and ``faces``, or a TriIndex)."""
    if isinstance(mesh, TriIndex):
        index = mesh
    else:
        index = TriIndex(*cuda_verts_faces(mesh, points.device if torch.is_tensor(points) and points.is_cuda else None))
    if not torch.is_tensor(points):
        points = torch.as_tensor(np.asarray(points), dtype=torch.float32).reshape(-1, 3)
    dist, face, closest = index.query(points.to(index.device))
    return closest, dist, face


@torch.no_grad()
def distance_p2m(points, mesh):
    """eval_rec.py:120-129: the distance of each point to the mesh [m] float64."""
    return closest_point(mesh, points)[1]


def _transform(p, T):
    """p [n, 3] float64 -> R p + t, as ((R0 x + R1 y) + R2 z) + t with every operation rounded on its own."""
    R, t = T[:3, :3], T[:3, 3]
    cols = [((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k] for k in range(3)]
    return torch.stack(cols, -1)


def _kabsch(src, tgt, with_scaling=False):
    """4x4 minimising |c R src + t - tgt| (Eigen::umeyama, as open3d's TransformationEstimationPointToPoint): rigid (c = 1)
    unless ``with_scaling``, then c = trace(D S) / mean |src - mean src|^2 with D the singular values of the cross-covariance.
    float64 sums on the device, the 3x3 SVD on the host."""
    ms, mt = src.mean(0), tgt.mean(0)
    cov = ((tgt - mt).T @ (src - ms)) / src.shape[0]
    parts = [ms, mt, cov.reshape(-1)]
    if with_scaling:
        ds = src - ms
        parts.append(((ds * ds).sum() / src.shape[0]).reshape(1))
    sums = torch.cat(parts).cpu().numpy()
    ms, mt, cov = sums[:3], sums[3:6], sums[6:15].reshape(3, 3)
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    if with_scaling:
        if not sums[15] > 0:
            raise ValueError("icp_point_to_point: the matched source points coincide; no scale can be estimated")
        R = ((D[0] * S[0, 0] + D[1] * S[1, 1]) + D[2] * S[2, 2]) / sums[15] * R
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mt - R @ ms
    return T


@torch.no_grad()
def icp_point_to_point(source, target, max_corr=0.1, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, index=None,
                       with_scaling=False):
    """open3d's registration_icp(source, target, max_corr, init, TransformationEstimationPointToPoint()) with default
    ICPConvergenceCriteria (eval_rec.py:190-204).  Correspondences: each source point's nearest target with d2 <
    fp32(max_corr^2); fitness = correspondences / source points; inlier_rmse = sqrt(mean of the squared correspondence
    distances) (both 0 without correspondences).  Each iteration left-multiplies the Kabsch update onto the transformation and
    moves the float64 source by it; it stops when |d fitness| < rel_fitness and |d rmse| < rel_rmse, or after max_iter.
    ``with_scaling``: every update is Umeyama WITH scale (open3d's TransformationEstimationPointToPoint(with_scaling=True),
    CloudCompare's -ADJUST_SCALE), so the transformation is a similarity; everything else in the loop is unchanged.
    Returns dict(transformation [4,4] float64 numpy, fitness, inlier_rmse, iterations).  ``index``: a prebuilt NNIndex of target."""
    src = checked_points(source, "icp_point_to_point").double()
    if src.shape[0] == 0:
        raise ValueError("icp_point_to_point: empty source")
    tgt = checked_points(target, "icp_point_to_point").double()
    index = index if index is not None else NNIndex(target)
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4).copy()
    cur = _transform(src, torch.from_numpy(T).to(src.device))

    def evaluate(p):
        d, i = index.query(p.float(), max_corr)
        ok = i >= 0
        k = int(ok.sum())
        if k == 0:
            return 0.0, 0.0, ok, i
        d64 = d[ok].double()
        return k / p.shape[0], math.sqrt(float((d64 * d64).sum()) / k), ok, i

    fit, rmse, ok, i = evaluate(cur)
    it = 0
    for it in range(max_iter):
        if int(ok.sum()) == 0:
            upd = np.eye(4)
        else:
            upd = _kabsch(cur[ok], tgt[i[ok]], with_scaling)
        T = upd @ T
        cur = _transform(cur, torch.from_numpy(upd).to(src.device))
        prev = (fit, rmse)
        fit, rmse, ok, i = evaluate(cur)
        if abs(prev[0] - fit) < rel_fitness and abs(prev[1] - rmse) < rel_rmse:
            break
    return dict(transformation=T, fitness=fit, inlier_rmse=rmse, iterations=it + 1 if max_iter > 0 else 0)


def _face_normals(v, f):
    """unit face normals [F, 3] float64 (trimesh's face_normals; sampled faces never have zero area)"""
    v = v.double()
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    n = torch.linalg.cross(e1, e2)
    return n / n.norm(dim=-1, keepdim=True).clamp_min(1e-300)


@torch.no_grad()
def mesh_metrics(rec, gt, n_points=200000, seed=0, align=True, scale=1.0, device="cuda", pre_transform=None, clean=None,
                 region=None, adjust_scale=False, cull=None, surface="samples", connectivity="vertex", icp="point"):
    """calc_3d_metric + calc_normal_consistency of eval_rec.py on the device.  ``rec`` / ``gt``: dicts with ``verts`` [V,3] and
    ``faces`` [F,3] (numpy or torch; what read_ply / marching_cubes return).  Both are divided by ``scale``; with ``align`` the
    reconstruction is moved by ICP of its vertices onto the ground truth's (max_corr 0.1).  n_points samples per surface (seeds
    ``seed`` for rec, ``seed + 1`` for gt).  Returns, in scene units: accuracy, completion, completion ratio (< 0.05),
    normals (mean |dot| of the face normals, both directions), chamfer-L1, chamfer-L2, f-score / f-score-15 / f-score-20
    (thresholds 0.010 / 0.015 / 0.020, <=), and transformation / icp fitness / icp rmse.
    Departure: one ICP and one sample set per mesh serve every metric (the reference draws and aligns twice).
    The steps eval_rec.py's __main__ (:259-272) does before the metrics, in its order, each off by default:
    ``pre_transform`` (4x4 similarity, alignment_transformation_sim3.npy) moves the scaled reconstruction; ``clean``
    ("largest", or "touching" / "not_touching" with ``region`` = (lo, hi)) keeps those components of it
    (mesh_clean.keep_components) and adds "components" (count before cleaning) and "kept area fraction" to the result;
    ``connectivity`` ("vertex", the default, or "edge") is keep_components' rule for what a component is;
    ``adjust_scale`` lets the ICP estimate a scale as well.  Departure: that one ICP does what CloudCompare's
    -ICP -ADJUST_SCALE and open3d's registration_icp do one after the other in the reference.
    ``cull`` (off by default; not a step of the reference): dict(c2w=, intrinsics=, size=(H, W) [, mode=, rel=, near=, method=]) keeps the faces of
    the reconstruction that some of these cameras saw (mesh_render.cull_mesh), after ``pre_transform`` and ``clean`` and
    before the ICP, and adds "culled face fraction" to the result.  The cameras look at the reconstruction AS IT IS AT THAT POINT: the
    poses (and the default near of 0.01) are in the frame and units the vertices have after the division by ``scale`` and after
    ``pre_transform`` -- with ``scale`` other than 1, poses in the mesh file's own units would look at a mesh of another size.
    ``surface``: "samples" (the default, the reference's numbers) measures each sample against the other surface's SAMPLES; "mesh"
    (not a step of the reference, which carries distance_p2m unused) measures it against the other MESH: the same samples from
    the same seeds, accuracy = mean distance of the reconstruction's samples to the ground-truth mesh, completion = mean distance
    of the ground truth's samples to the reconstruction's mesh, the normals term against the closest face's normal, everything
    else from those two distance arrays (metrics_from_surfaces); the result then carries "surface": "mesh".
    ``icp``: what the alignment minimises.  "point" (the default, the reference's): icp_point_to_point.
    "plane": mesh_register.icp_point_to_plane of the reconstruction's vertices against the ground truth's vertices with
    mesh_smooth.vertex_normals(gt, "angle"); "surface": against the ground-truth MESH itself.  Both are rigid, so either
    with ``adjust_scale`` raises ValueError; the result then carries "icp": the metric, and "icp degenerate"."""
    if surface not in ("samples", "mesh"):
        raise ValueError(f"mesh_metrics: surface must be 'samples' or 'mesh', got {surface!r}")
    if icp not in ("point", "plane", "surface"):
        raise ValueError(f"mesh_metrics: icp must be 'point', 'plane' or 'surface', got {icp!r}")
    if icp != "point" and adjust_scale:
        raise ValueError(f"mesh_metrics: icp={icp!r} is rigid; adjust_scale goes with icp='point' only")
    need_gpu("mesh_metrics")
    rv, rf = cuda_verts_faces(rec, device, cast=True)
    gv, gf = cuda_verts_faces(gt, device, cast=True)
    if rv.shape[0] == 0 or rf.shape[0] == 0:
        raise ValueError("mesh_metrics: empty reconstruction")
    if gv.shape[0] == 0 or gf.shape[0] == 0:
        raise ValueError("mesh_metrics: empty ground truth")
    rv, gv = (rv.double() / scale).float(), (gv.double() / scale).float()
    extra = {}
    if pre_transform is not None or clean is not None:
        from . import mesh_clean                             # (a cycle: mesh_clean moves vertices with _transform)
        if pre_transform is not None:
            _, P = mesh_clean.check_similarity(pre_transform)
            rv = _transform(rv.double(), torch.from_numpy(P).to(rv.device)).float()
        if clean is not None:
            kept, st = mesh_clean.keep_components({"verts": rv, "faces": rf}, clean, region, device, connectivity=connectivity)
            rv, rf = kept["verts"], kept["faces"]
            extra = {"components": st["n_components"], "kept area fraction": st["kept_area_fraction"]}
    if cull is not None:
        from . import mesh_render                            # (a cycle: mesh_render -> mesh_clean -> this module)
        n_before = rf.shape[0]
        kept = mesh_render.cull_mesh({"verts": rv, "faces": rf}, **cull)
        rv, rf = kept["verts"], kept["faces"]
        if rf.shape[0] == 0:
            raise ValueError("mesh_metrics: culling left no face of the reconstruction")
        extra["culled face fraction"] = 1.0 - rf.shape[0] / n_before
    T, fit, rmse = np.eye(4), None, None
    if align:
        if icp == "point":
            res = icp_point_to_point(rv, gv, 0.1, with_scaling=adjust_scale)
        else:
            from . import mesh_register, mesh_smooth         # (cycles: both are built on this module's indexes)
            if icp == "plane":
                gn = mesh_smooth.vertex_normals({"verts": gv, "faces": gf.to(torch.int32)}, "angle")
                res = mesh_register.icp_point_to_plane(rv, gv, gn, 0.1)
            else:
                res = mesh_register.icp_point_to_plane(rv, (gv, gf), None, 0.1)
            extra.update({"icp": icp, "icp degenerate": res["degenerate"]})
        T, fit, rmse = res["transformation"], res["fitness"], res["inlier_rmse"]
        rv = _transform(rv.double(), torch.from_numpy(T).to(rv.device)).float()
    rp, ri = sample_surface(rv, rf, n_points, seed)
    gp, gi = sample_surface(gv, gf, n_points, seed + 1)
    if surface == "mesh":
        out = metrics_from_surfaces(rp, _face_normals(rv, rf)[ri], (rv, rf), gp, _face_normals(gv, gf)[gi], (gv, gf))
    else:
        out = metrics_from_samples(rp, _face_normals(rv, rf)[ri], gp, _face_normals(gv, gf)[gi])
    out.update({"transformation": T, "icp fitness": fit, "icp rmse": rmse})
    out.update(extra)
    return out


@torch.no_grad()
def metrics_from_samples(rec_pts, rec_normals, gt_pts, gt_normals):
    """eval_pointcloud / calc_3d_metric arithmetic on two sample sets (fp32 points, float64 unit normals)."""
    d_acc, i_acc = nearest(rec_pts, gt_pts)          # accuracy: reconstruction -> ground truth
    d_com, i_com = nearest(gt_pts, rec_pts)          # completion: ground truth -> reconstruction
    acc, com = d_acc.double(), d_com.double()
    n_acc = (gt_normals[i_acc] * rec_normals).sum(-1).abs().mean()
    n_com = (rec_normals[i_com] * gt_normals).sum(-1).abs().mean()
    out = {"accuracy": float(acc.mean()), "completion": float(com.mean()),
           "completion ratio": float((com < COMPLETION_RATIO_THRESHOLD).double().mean()),
           "normals": float(0.5 * n_com + 0.5 * n_acc),
           "chamfer-L1": float(0.5 * (com.mean() + acc.mean())),
           "chamfer-L2": float(0.5 * ((com * com).mean() + (acc * acc).mean()))}
    for key, th in zip(("f-score", "f-score-15", "f-score-20"), F_THRESHOLDS):
        p, r = float((acc <= th).double().mean()), float((com <= th).double().mean())
        out[key] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return out


def surface_metrics(d_acc, d_com, dot_acc, dot_com):
    """The surface="mesh" arithmetic on float64 tensors (any device): ``d_acc`` the distances of the reconstruction's samples to
    the ground-truth mesh, ``d_com`` those of the ground truth's samples to the reconstruction's mesh, ``dot_*`` the products
    n_sample . n_closest_face of the same pairs.  Thresholds and comparisons are those of metrics_from_samples."""
    acc, com = d_acc.double(), d_com.double()
    out = {"accuracy": float(acc.mean()), "completion": float(com.mean()),
           "completion ratio": float((com < COMPLETION_RATIO_THRESHOLD).double().mean()),
           "normals": float(0.5 * dot_com.double().abs().mean() + 0.5 * dot_acc.double().abs().mean()),
           "chamfer-L1": float(0.5 * (com.mean() + acc.mean())),
           "chamfer-L2": float(0.5 * ((com * com).mean() + (acc * acc).mean()))}
    for key, th in zip(("f-score", "f-score-15", "f-score-20"), F_THRESHOLDS):
        p, r = float((acc <= th).double().mean()), float((com <= th).double().mean())
        out[key] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    out["surface"] = "mesh"
    return out


@torch.no_grad()
def metrics_from_surfaces(rec_pts, rec_normals, rec_mesh, gt_pts, gt_normals, gt_mesh, acc=None, com=None):
    """The metrics of mesh_metrics(surface="mesh") on given samples (fp32 points, float64 unit normals) and meshes ((verts, faces)
    CUDA tensors): accuracy from rec_pts against gt_mesh, completion from gt_pts against rec_mesh, the normals term
    |n_sample . n_face| with n_face the unit normal of the closest face.  ``acc`` / ``com``: (dist, face) to use in place of the
    two queries (a test feeds an oracle's)."""
    d_acc, f_acc = acc if acc is not None else TriIndex(*gt_mesh).query(rec_pts)[:2]
    d_com, f_com = com if com is not None else TriIndex(*rec_mesh).query(gt_pts)[:2]
    if bool((f_acc < 0).any()) or bool((f_com < 0).any()):
        raise ValueError("metrics_from_surfaces: a sample has no closest face (non-finite sample, or a mesh without a usable face)")
    gn, rn = _face_normals(gt_mesh[0], gt_mesh[1].long()), _face_normals(rec_mesh[0], rec_mesh[1].long())
    return surface_metrics(d_acc, d_com, (gn[f_acc] * rec_normals).sum(-1), (rn[f_com] * gt_normals).sum(-1))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_eval", description=__doc__.splitlines()[0])
    ap.add_argument("rec")
    ap.add_argument("gt")
    ap.add_argument("--no-align", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sim3", metavar="T.npy", help="4x4 similarity applied to REC first (alignment_transformation_sim3.npy)")
    ap.add_argument("--clean", choices=("largest", "touching", "not_touching"), help="keep these components of REC")
    ap.add_argument("--region", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--connectivity", choices=("vertex", "edge"), default="vertex",
                    help="with --clean: faces joined at a shared vertex (the default) or only across a shared edge")
    ap.add_argument("--adjust-scale", action="store_true", help="the ICP estimates a scale as well")
    ap.add_argument("--cull-poses", metavar="POSES", help="cull REC to what these camera-to-world poses saw (.npy, text or a directory); the poses are in the frame REC has "
                    "after --scale and --sim3 have been applied, not in the file's own units")
    ap.add_argument("--cull-intrinsics", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"))
    ap.add_argument("--cull-size", type=int, nargs=2, metavar=("H", "W"))
    ap.add_argument("--cull-mode", choices=("any", "all", "frustum"), default="any")
    ap.add_argument("--cull-raycast", action="store_true", help="decide visibility by casting rays (mesh_render method='raycast')")
    ap.add_argument("--surface", choices=("samples", "mesh"), default="samples",
                    help="measure each sample against the other surface's samples (the reference) or against the other mesh itself")
    ap.add_argument("--icp", choices=("point", "plane", "surface"), default="point",
                    help="what the alignment minimises: point to point (the reference), point to plane against GT's vertices and "
                    "normals, or point to plane against GT's surface itself")
    a = ap.parse_args(argv)
    if a.icp != "point" and a.adjust_scale:
        ap.error("--adjust-scale goes with --icp point only")
    if a.cull_poses and not (a.cull_intrinsics and a.cull_size):
        ap.error("--cull-poses needs --cull-intrinsics and --cull-size")
    if not a.cull_poses and (a.cull_intrinsics or a.cull_size):
        ap.error("--cull-intrinsics and --cull-size go with --cull-poses")
    cull = None
    if a.cull_poses:
        from .mesh_render import read_poses                  # (the cycle named in mesh_metrics)
        cull = dict(c2w=read_poses(a.cull_poses), intrinsics=a.cull_intrinsics, size=tuple(a.cull_size), mode=a.cull_mode)
        if a.cull_raycast:
            cull["method"] = "raycast"
    if (a.clean in ("touching", "not_touching")) != (a.region is not None):
        ap.error("--region goes with --clean touching or not_touching, and they need it")
    m = mesh_metrics(read_ply(a.rec), read_ply(a.gt), a.points, a.seed, not a.no_align, a.scale,
                     pre_transform=np.load(a.sim3) if a.sim3 else None, clean=a.clean,
                     region=(a.region[:3], a.region[3:]) if a.region else None, adjust_scale=a.adjust_scale, cull=cull,
                     surface=a.surface, connectivity=a.connectivity, icp=a.icp)
    if a.surface == "mesh":
        print("surface: mesh (each sample against the other mesh's surface)")
    print("accuracy: ", m["accuracy"] * 100, "cm")
    print("completion: ", m["completion"] * 100, "cm")
    print("completion ratio: ", m["completion ratio"] * 100, "%")
    print("Normal Consistency", f"{m['normals'] * 100:.4f} %")
    for k in ("chamfer-L1", "chamfer-L2", "f-score", "f-score-15", "f-score-20", "icp fitness", "icp rmse"):
        print(f"{k}: {m[k]}")
    print("transformation:\n" + np.array2string(m["transformation"], precision=8))
    if "components" in m:
        print(f"components: {m['components']}  kept area fraction: {m['kept area fraction']}")
    if "culled face fraction" in m:
        print(f"culled face fraction: {m['culled face fraction']}")
    return m


if __name__ == "__main__":
    main()
