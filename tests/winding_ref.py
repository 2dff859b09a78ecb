"""numpy float64 oracle of the generalised winding number (include/nicer_slam_amd.h Section 16, csrc/mesh_winding.hip): the solid
angle of a face, the tree with the header's build and visiting order, the exact sum and the tree walk with their counts and the
smallest relative gap of the decisions a query made; plus the meshes the tests share.  numpy rounds every elementwise operation on its
own, which is the contract."""
import numpy as np

import p2m_ref as P
from sdf_ref import _cross

FOUR_PI = float.fromhex("0x1.921fb54442d18p+3")
MAX_LEVEL = 10


def solid_angle(q, a, b, c):
    """Omega of faces (a, b, c) from q, broadcast (Van Oosterom & Strackee); 0 where det == 0"""
    with np.errstate(all="ignore"):
        A, B, C = a - q, b - q, c - q
        lA, lB, lC = np.sqrt(P._dot(A, A)), np.sqrt(P._dot(B, B)), np.sqrt(P._dot(C, C))
        det = P._dot(A, _cross(B, C))
        den = ((lA * lB) * lC + P._dot(A, B) * lC) + (P._dot(A, C) * lB + P._dot(B, C) * lA)
        return np.where(det == 0, 0.0, 2.0 * np.arctan2(det, den))


def level_of(n):
    L = 0
    while L < MAX_LEVEL and 8 * 4 ** L < n:
        L += 1
    return L


def max_nodes(F):
    return sum(min(8 ** l, F) for l in range(level_of(F) + 1))


def _morton(cell, L):
    key = np.zeros(cell.shape[0], np.int64)
    for bit in range(L):
        for k in range(3):
            key |= ((cell[:, k] >> bit) & 1) << (3 * bit + (2 - k))
    return key


class Tree:
    """the tree of Section 16 over (verts, faces): the sorted usable faces (``face`` their indices, ``a``, ``b``, ``c`` their float64
    vertices) and the nodes in pre-order: level, begin, end, skip, leaf, N, area, M, P, r2"""

    def __init__(self, verts, faces):
        v = np.asarray(verts, np.float32).astype(np.float64)
        f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
        use = np.nonzero(P.face_causes(verts, f) == 0)[0]
        self.F, self.n_usable = f.shape[0], use.size
        self.L = L = level_of(use.size)
        self.n_nodes = 0
        self.face = use
        self.a = self.b = self.c = np.zeros((0, 3))
        if use.size == 0:
            return
        a, b, c = v[f[use, 0]], v[f[use, 1]], v[f[use, 2]]
        corners = np.concatenate([a, b, c])
        lo = corners.min(0) + 0.0
        side = (corners.max(0) - corners.min(0)).max()
        scale = float(1 << L) / side
        cen = ((a + b) + c) / 3.0
        cell = np.minimum(np.maximum((cen - lo) * scale, 0.0), float((1 << L) - 1)).astype(np.int64)
        key = _morton(cell, L)
        order = np.argsort(key, kind="stable")
        self.face, self.key = use[order], key[order]
        self.a, self.b, self.c, cen = a[order], b[order], c[order], cen[order]
        n = use.size
        # h(i): at how many levels position i begins a node; base: its exclusive prefix sum
        h = np.zeros(n + 1, np.int64)
        h[0] = L + 1
        x = self.key[1:] ^ self.key[:-1]
        msb = np.array([int(t).bit_length() - 1 for t in x], np.int64)
        h[1:n] = np.where(x != 0, msb // 3 + 1, 0)
        base = np.concatenate([[0], np.cumsum(h)])[:n + 1]
        self.n_nodes = K = int(h.sum())
        assert K <= max_nodes(self.F)
        self.level, self.begin, self.end = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
        self.skip = np.zeros(K, np.int64)
        prefix = [self.key >> (3 * (L - l)) for l in range(L + 1)]
        for i in np.nonzero(h[:n])[0]:
            lmin = L + 1 - h[i]
            for l in range(lmin, L + 1):
                k = base[i] + (l - lmin)
                e = int(np.searchsorted(prefix[l], prefix[l][i], side="right"))
                self.level[k], self.begin[k], self.end[k], self.skip[k] = l, i, e, base[e]
        self.leaf = self.level == L
        # moments: leaves over their faces in sorted order, parents over their children in ascending key order, every sum from +0
        nt = _cross(self.b - self.a, self.c - self.a) * 0.5
        at = np.sqrt((nt[:, 0] * nt[:, 0] + nt[:, 1] * nt[:, 1]) + nt[:, 2] * nt[:, 2])
        self.N, self.M, self.area = np.zeros((K, 3)), np.zeros((K, 3)), np.zeros(K)
        by_start = {(int(self.level[k]), int(self.begin[k])): k for k in range(K)}
        for l in range(L, -1, -1):
            for k in np.nonzero(self.level == l)[0]:
                s, e = self.begin[k], self.end[k]
                N, M, area = np.zeros(3), np.zeros(3), 0.0
                if l == L:
                    for t in range(s, e):
                        area = area + at[t]
                        N = N + nt[t]
                        M = M + at[t] * cen[t]
                else:
                    j = s
                    while j < e:
                        ch = by_start[(l + 1, int(j))]
                        area = area + self.area[ch]
                        N = N + self.N[ch]
                        M = M + self.M[ch]
                        j = self.end[ch]
                self.N[k], self.M[k], self.area[k] = N, M, area
        self.P = self.M / self.area[:, None]
        self.r2 = np.zeros(K)
        for k in range(K):
            s, e = self.begin[k], self.end[k]
            x = np.concatenate([self.a[s:e], self.b[s:e], self.c[s:e]]) - self.P[k]
            self.r2[k] = P._dot(x, x).max()


def _tree(mesh_or_tree, faces=None):
    return mesh_or_tree if isinstance(mesh_or_tree, Tree) else Tree(mesh_or_tree, faces)


def exact(queries, tree, flip=False, pairs=400_000):
    """dict(w, evaluated, accepted, abs): the exact sum over the usable faces in the tree's sorted order; ``abs`` = sum |Omega| / 4 pi"""
    q = np.asarray(queries, np.float32).astype(np.float64).reshape(-1, 3)
    M, n = q.shape[0], tree.n_usable
    S, A = np.zeros(M), np.zeros(M)
    if n:
        step = max(1, pairs // n)
        for lo in range(0, M, step):
            om = solid_angle(q[lo:lo + step, None, :], tree.a[None], tree.b[None], tree.c[None])
            S[lo:lo + step] = 0.0 + np.cumsum(om, 1)[:, -1]                  # cumsum: in order, one by one
            A[lo:lo + step] = np.abs(om).sum(1)
    w = S / FOUR_PI
    if flip:
        w = -w
    bad = ~np.isfinite(q).all(1)
    w[bad] = np.nan
    return dict(w=w, evaluated=np.where(bad, 0, n), accepted=np.zeros(M, np.int64), abs=A / FOUR_PI)


def walk(queries, tree, beta=2.0, flip=False):
    """dict(w, accepted, evaluated, gap, abs): the pre-order walk of every query (in lockstep, one node per query and round);
    ``gap`` = the smallest |d2 - beta^2 r2| / d2 over the decisions the query made (inf when it made none), ``abs`` = the sum of
    the absolute terms / 4 pi"""
    assert beta >= 1.0
    q = np.asarray(queries, np.float32).astype(np.float64).reshape(-1, 3)
    M = q.shape[0]
    beta2 = beta * beta
    S, A = np.zeros(M), np.zeros(M)
    acc, ev = np.zeros(M, np.int64), np.zeros(M, np.int64)
    gap = np.full(M, np.inf)
    i = np.zeros(M, np.int64)
    finite = np.isfinite(q).all(1)
    with np.errstate(all="ignore"):
        while True:
            idx = np.nonzero(finite & (i < tree.n_nodes))[0]
            if idx.size == 0:
                break
            n = i[idx]
            d = tree.P[n] - q[idx]
            d2 = P._dot(d, d)
            thr = beta2 * tree.r2[n]
            g = np.abs(d2 - thr) / d2
            gap[idx] = np.minimum(gap[idx], np.where(np.isnan(g), np.inf if np.isinf(beta2) else 0.0, g))
            accept = d2 > thr
            ia, na = idx[accept], n[accept]
            term = P._dot(tree.N[na], d[accept]) / (d2[accept] * np.sqrt(d2[accept]))
            S[ia] = S[ia] + term
            A[ia] += np.abs(term)
            acc[ia] += 1
            i[ia] = tree.skip[na]
            leaf = ~accept & tree.leaf[n]
            il, nl = idx[leaf], n[leaf]
            count = tree.end[nl] - tree.begin[nl]
            for t in range(int(count.max()) if count.size else 0):
                sel = count > t
                pos = tree.begin[nl[sel]] + t
                om = solid_angle(q[il[sel]], tree.a[pos], tree.b[pos], tree.c[pos])
                S[il[sel]] = S[il[sel]] + om
                A[il[sel]] += np.abs(om)
                ev[il[sel]] += 1
            i[idx[~accept]] += 1
    w = S / FOUR_PI
    if flip:
        w = -w
    w[~finite] = np.nan
    return dict(w=w, accepted=acc, evaluated=ev, gap=gap, abs=A / FOUR_PI)


# ---- shared meshes ----------------------------------------------------------------------------------------------------------------

def holed_sphere(rows=5, n_lat=24, n_lon=48):
    """P.latlong_sphere without its top ``rows`` latitude rows: a hole of rows * 180 / n_lat degrees half-angle about +z (37.5)"""
    v, f, _ = P.latlong_sphere(n_lat, n_lon)
    return v, f[2 * n_lon * rows:]


HOLE_QUERIES = np.array([[0, 0, 0.85], [0, 0, 1.0], [0, 0, 1.1], [0, 0, 1.2], [0.2, 0.1, 0.9], [0.2, 0.1, 1.0], [0.2, 0.1, 1.1]],
                        np.float32)


def opposite_twins():
    """two coincident faces of opposite winding"""
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 1]], np.int32)


def coincident_copies(k=40):
    """k copies of one triangle: one leaf at L >= 1"""
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.tile(np.array([[0, 1, 2]], np.int32), (k, 1))


def cube_queries(n=4097, seed=0, half=1.5):
    return np.random.default_rng(seed).uniform(-half, half, (n, 3)).astype(np.float32)
