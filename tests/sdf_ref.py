"""numpy float64 oracle of the signed and range-limited closest-point query (include/nicer_slam_amd.h Section 15, csrc/mesh_sdf.hip),
built on tests/p2m_ref.py: the brute-force winner of Section 14 with its float64 closest point, the feature code, the
angle-weighted pseudo-normal N and its weight W from a numpy vertex -> face list, the sign and the bound; plus the meshes the
tests share."""
import numpy as np

import p2m_ref as P


def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def _len(n):
    return np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])


def pair_feature(q, a, b, c):
    """the feature code of float64 q against faces (a, b, c), broadcast: the first test of Section 14's classification that holds"""
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = q - a, q - b, q - c
        d1, d2, d3, d4, d5, d6 = P._dot(ab, ap), P._dot(ac, ap), P._dot(ab, bp), P._dot(ac, bp), P._dot(ab, cp), P._dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        return np.select(tests, [1, 2, 3, 4, 5, 6], 0).astype(np.int8)


def weld_faces(verts, faces):
    """the adjacency faces TriIndex builds with weld=True: every in-range index replaced by the rank of its vertex's fp32
    coordinates among the distinct ones (-0 = +0; a non-finite vertex counts as (0, 0, 0)); a face with an index outside [0, V) is kept
    as it is"""
    v = np.asarray(verts, np.float32) + np.float32(0.0)
    v = np.where(np.isfinite(v).all(1, keepdims=True), v, np.float32(0.0))      # (as TriIndex.adjacency: such a vertex's name is moot)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    _, inverse = np.unique(v, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    ok = ((f >= 0) & (f < v.shape[0])).all(1)
    out = f.copy()
    out[ok] = inverse[f[ok]]
    return out.astype(np.int32)


class Tables:
    """per mesh: which faces contribute, their unit normals, corner angles, and the corner lists by adjacency vertex"""

    def __init__(self, verts, faces, adj):
        v = np.asarray(verts, np.float32).astype(np.float64)
        f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
        self.adj = np.asarray(adj).astype(np.int64).reshape(-1, 3)
        V, F = v.shape[0], f.shape[0]
        assert self.adj.shape[0] == F
        usable = P.face_causes(verts, f) == 0
        self.contributes = usable & ((self.adj >= 0) & (self.adj < V)).all(1)
        fs = np.where(usable[:, None], f, 0)
        x = np.stack([v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]], 1)                    # [F, 3 corners, 3]
        with np.errstate(all="ignore"):
            n = _cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
            self.nhat = n / _len(n)[:, None]
            self.alpha = np.zeros((F, 3))
            for k in range(3):
                u, w = x[:, (k + 1) % 3] - x[:, k], x[:, (k + 2) % 3] - x[:, k]
                self.alpha[:, k] = np.arctan2(_len(_cross(u, w)), P._dot(u, w))
        # corners 3 g + k of the contributing faces, sorted by adjacency vertex, ascending within a vertex (stable)
        corners = np.nonzero(np.repeat(self.contributes, 3))[0]
        keys = self.adj.reshape(-1)[corners]
        order = np.argsort(keys, kind="stable")
        self.corner = corners[order]
        self.start = np.searchsorted(keys[order], np.arange(V + 1))
        self.V = V

    def corners_at(self, i):
        if not 0 <= i < self.V:
            return self.corner[:0]
        return self.corner[self.start[i]:self.start[i + 1]]

    def vertex(self, i):
        c = self.corners_at(i)
        if c.size == 0:
            return np.zeros(3), 0.0
        al = self.alpha[c // 3, c % 3]
        return np.cumsum(al[:, None] * self.nhat[c // 3], 0)[-1], float(np.cumsum(al)[-1])       # cumsum: in order, one by one

    def edge(self, i, j):
        g = np.unique(self.corners_at(i) // 3)                                   # ascending, each face once
        g = g[(self.adj[g] == j).any(1)] if 0 <= j < self.V else g[:0]
        if g.size == 0:
            return np.zeros(3), 0.0
        return np.cumsum(self.nhat[g], 0)[-1], float(g.size)


def winner(queries, verts, faces, pairs=400_000):
    """(face [M] int64, d2 [M] float64, p [M, 3] float64, feature [M] int8) by brute force: P.closest_brute with the closest point
    kept in float64 and the feature of the winning pair"""
    q = np.asarray(queries, np.float32).astype(np.float64).reshape(-1, 3)
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    use = np.nonzero(P.face_causes(verts, f) == 0)[0]
    M = q.shape[0]
    face = np.full(M, -1, np.int64)
    best = np.full(M, np.inf)
    p64 = np.full((M, 3), np.nan)
    feature = np.full(M, -1, np.int8)
    if use.size:
        a, b, c = v[f[use, 0]], v[f[use, 1]], v[f[use, 2]]
        step = max(1, pairs // use.size)
        for lo in range(0, M, step):
            qq = q[lo:lo + step]
            p, d2 = P.pair_closest(qq[:, None, :], a[None], b[None], c[None])
            d2 = np.where(np.isnan(d2), np.inf, d2)
            k = d2.argmin(1)
            rows = np.arange(k.size)
            found = d2[rows, k] < np.inf
            best[lo:lo + step] = d2[rows, k]
            face[lo:lo + step] = np.where(found, use[k], -1)
            p64[lo:lo + step] = np.where(found[:, None], p[rows, k], np.nan)
            feature[lo:lo + step] = np.where(found, pair_feature(qq, a[k], b[k], c[k]), -1)
    bad = ~np.isfinite(q).all(1)
    face[bad] = -1
    best[bad] = np.nan
    p64[bad] = np.nan
    feature[bad] = -1
    return face, best, p64, feature


_CORNERS = {1: (0,), 2: (1,), 4: (2,), 3: (0, 1), 5: (0, 2), 6: (1, 2)}


def signed_brute(queries, verts, faces, adj=None, weld=True, flip=False, max_d2=np.inf):
    """dict of the contract's outputs for every query: face int64, d2 float64, closest fp32, feature int8, N [M, 3], W, sign int8 and
    -- for the tests' margins -- edotn = e . N and enorm = |e|.  ``adj``: adjacency faces (default: welded, or the faces themselves)."""
    assert max_d2 >= 0
    q = np.asarray(queries, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    if adj is None:
        adj = weld_faces(verts, f) if weld else f
    T = Tables(verts, f, adj)
    face, d2, p, feature = winner(q, verts, f)
    M = q.shape[0]
    with np.errstate(invalid="ignore"):
        out_of_range = (face >= 0) & (d2 > max_d2)
    face[out_of_range] = -1
    d2[out_of_range] = np.inf
    p[out_of_range] = np.nan
    feature[out_of_range] = -1
    N, W = np.zeros((M, 3)), np.zeros(M)
    for m in np.nonzero(face >= 0)[0]:
        g, ft = face[m], int(feature[m])
        if ft == 0:
            N[m], W[m] = T.nhat[g], 1.0
        elif len(_CORNERS[ft]) == 1:
            N[m], W[m] = T.vertex(T.adj[g, _CORNERS[ft][0]])
        else:
            N[m], W[m] = T.edge(T.adj[g, _CORNERS[ft][0]], T.adj[g, _CORNERS[ft][1]])
    e = np.where(face[:, None] >= 0, q - p, 0.0)
    edotn = P._dot(e, N)
    sign = np.where(edotn < 0, -1, 1).astype(np.int8)
    if flip:
        sign = (-sign).astype(np.int8)
    with np.errstate(over="ignore", invalid="ignore"):
        closest = p.astype(np.float32)
    return dict(face=face, d2=d2, closest=closest, feature=feature, N=N, W=W, sign=sign, edotn=edotn, enorm=_len(e), p=p,
                dist=sign * np.sqrt(d2))


def closest_face_sign(queries, verts, faces, ref):
    """the naive rule: the sign of (q - p) . n of the closest face (+1 at zero), for the oracle's winners ``ref``"""
    q = np.asarray(queries, np.float32).astype(np.float64).reshape(-1, 3)
    n = P.face_normals(verts, np.asarray(faces)[np.maximum(ref["face"], 0)])
    return np.where(P._dot(q - ref["p"], n) < 0, -1, 1)


# ---- shared meshes ----------------------------------------------------------------------------------------------------------------

def spike(K=40, half=0.1, hgt=1.0):
    """(verts fp32, faces int32, apex vertex index, the four outward unit side normals [4, 3]): a closed four-sided pyramid of height
    ``hgt`` and half-angle ``half`` at the apex -- base corners (+-w, +-w, 0), w = hgt tan(half), counter-clockwise seen from above --
    whose side 2 (opposite side 0) is split into K slivers through the apex, with a base fan from corner 0 that uses every base
    vertex.  Outward winding.  The apex has K + 3 incident faces."""
    w = hgt * np.tan(half)
    c = np.array([[w, -w, 0], [w, w, 0], [-w, w, 0], [-w, -w, 0]], np.float64)
    mid = [c[2] + (c[3] - c[2]) * (i / K) for i in range(1, K)]
    ring = [c[0], c[1], c[2]] + mid + [c[3]]                     # the base polygon, counter-clockwise
    verts = np.array(ring + [[0, 0, hgt]], np.float32)
    apex = len(ring)
    n_ring = len(ring)
    faces = [[0, 1, apex], [1, 2, apex]]
    faces += [[i, i + 1, apex] for i in range(2, n_ring - 1)]    # side 2: K slivers
    faces += [[n_ring - 1, 0, apex]]
    faces += [[0, i + 1, i] for i in range(1, n_ring - 1)]       # the base fan, facing down
    normals = np.array([[hgt, 0, w], [0, hgt, w], [-hgt, 0, w], [0, -hgt, w]], np.float64)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    return verts, np.array(faces, np.int32), apex, normals


def open_square():
    """two triangles in z = 0 over [0, 1]^2, normals +z: an open surface"""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def three_on_an_edge():
    """three faces on the edge from (0, 0, 0) to (1, 0, 0): fins towards +y, +z and -y (a non-manifold edge)"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 0, 1], [0.5, -1, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int32)
