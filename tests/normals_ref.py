"""numpy statement of k nearest neighbours and of normal estimation from neighbourhoods (nicer_slam_amd/cloud_normals.py,
csrc/mesh_eval.hip k_nn_query_k, csrc/cloud_normals.hip, csrc/normals_passes.hpp; DESIGN 4za, header Section 28) for the tests.  Every
float64 operation is one numpy operation (+ - * / sqrt and comparisons), so each is rounded on its own; the device is held to these
functions bit for bit."""
import math

import numpy as np

MAX_SWEEPS = 16
NAN64 = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


# ---- k nearest neighbours -----------------------------------------------------------------------------------------------------------

def d2_f32(queries, targets):
    """fp32 d2 [m, n] = (dx*dx + dy*dy) + dz*dz with dk = t_k - q_k, each operation rounded (eval_ref.nn_brute's order)"""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    t = np.asarray(targets, np.float32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = (t[None, :, k] - q[:, None, k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


def knn_brute(queries, targets, k, max_dist=math.inf, chunk=256, d2_of=d2_f32, tie=1):
    """(dist fp32 [m, k], idx int64 [m, k], count int64 [m]): the k smallest targets under (d2, index), in that order; non-finite targets
    never chosen; with a radius only d2 < fp32(max_dist^2) counts; slots behind count hold (+inf, -1); a non-finite query gives count 0
    and (NaN, -1).  ``d2_of`` and ``tie`` (-1: ties to the higher index) are there for the tests' mutants."""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    t = np.asarray(targets, np.float32).reshape(-1, 3)
    m, n = len(q), len(t)
    valid = np.isfinite(t).all(1)
    strict = max_dist < math.inf
    r2 = np.float32(max_dist * max_dist) if strict else np.float32(np.inf)
    dist = np.full((m, k), np.inf, np.float32)
    idx = np.full((m, k), -1, np.int64)
    count = np.zeros(m, np.int64)
    ar = np.arange(n)
    for lo in range(0, m, chunk):
        d2 = d2_of(q[lo:lo + chunk], t)
        with np.errstate(invalid="ignore"):
            ok = valid[None, :] & ((d2 < r2) if strict else ~np.isnan(d2))
        masked = np.where(ok, d2, np.float32(np.inf))
        kth = np.partition(masked, k - 1, axis=1)[:, k - 1] if n > k else np.full(len(d2), np.inf, np.float32)
        for j in range(d2.shape[0]):
            cand = ar[ok[j] & (d2[j] <= kth[j])]               # (only a shortcut: everything up to the k-th smallest d2, ties included)
            order = np.lexsort((tie * cand, d2[j, cand]))[:k]
            c = len(order)
            idx[lo + j, :c] = cand[order]
            dist[lo + j, :c] = np.sqrt(d2[j, cand[order]].astype(np.float64)).astype(np.float32)
            count[lo + j] = c
    bad = ~np.isfinite(q).all(1)
    idx[bad] = -1
    dist[bad] = np.nan
    count[bad] = 0
    return dist, idx, count


# ---- one neighbourhood per row ------------------------------------------------------------------------------------------------------

def readable(n, idx, count):
    """rows whose first count slots all name a point: 1 <= count <= k and every one of them in [0, n)"""
    idx = np.asarray(idx, np.int64)
    count = np.asarray(count, np.int64)
    k = idx.shape[1]
    live = np.arange(k)[None, :] < count[:, None]
    return (count >= 1) & (count <= k) & ~(live & ((idx < 0) | (idx >= n))).any(1), live


def scatter(points, idx, count):
    """(S [m, 6] float64 = S00 S01 S02 S11 S12 S22, ok [m]): two passes over the neighbours in the order of idx, every sum started at +0.0
    and added left to right; rows that are not readable are NaN"""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    m, k = idx.shape
    ok, live = readable(len(p), idx, count)
    live = live & ok[:, None]
    safe = np.where(live, idx, 0)
    c = np.where(ok, np.asarray(count, np.int64), 1).astype(np.float64)
    pts = p[safe] if len(p) else np.zeros((m, k, 3))
    mu = np.zeros((m, 3))
    for j in range(k):
        mu = mu + np.where(live[:, j, None], pts[:, j], 0.0)
    mu = mu / c[:, None]
    S = np.zeros((m, 6))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for j in range(k):
        d = pts[:, j] - mu
        for s, (a, b) in enumerate(pairs):
            S[:, s] = S[:, s] + np.where(live[:, j], d[:, a] * d[:, b], 0.0)
    S[~ok] = np.nan
    return S, ok


def scatter_one_pass(points, idx, count):
    """MUTANT: sum p p^T - c mu mu^T in one pass"""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    m, k = idx.shape
    ok, live = readable(len(p), idx, count)
    pts = p[np.where(live & ok[:, None], idx, 0)]
    c = np.where(ok, np.asarray(count, np.int64), 1).astype(np.float64)
    w = (live & ok[:, None]).astype(np.float64)
    mu = (pts * w[:, :, None]).sum(1) / c[:, None]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    S = np.stack([(pts[:, :, a] * pts[:, :, b] * w).sum(1) - c * mu[:, a] * mu[:, b] for a, b in pairs], 1)
    S[~ok] = np.nan
    return S, ok


def _pivot(A, V, p, q):
    """one pivot of every row at once; A [m, 3, 3] symmetric (both triangles kept), V [m, 3, 3] = V[row, column]; returns g != 0"""
    r = 3 - p - q
    app, aqq, g, arp, arq = A[:, p, p].copy(), A[:, q, q].copy(), A[:, p, q].copy(), A[:, r, p].copy(), A[:, r, q].copy()
    with np.errstate(all="ignore"):
        nz = g != 0.0
        small = nz & (np.abs(app) + np.abs(g) == np.abs(app)) & (np.abs(aqq) + np.abs(g) == np.abs(aqq))
        rot = nz & ~small
        theta = (aqq - app) / (2.0 * g)
        at = np.abs(theta)
        t = np.where(at > 2.0 ** 500, 1.0 / (at + at), 1.0 / (at + np.sqrt(theta * theta + 1.0)))
        t = np.where(theta < 0.0, -t, t)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        h = t * g
        A[:, p, p] = np.where(rot, app - h, app)
        A[:, q, q] = np.where(rot, aqq + h, aqq)
        A[:, p, q] = A[:, q, p] = np.where(nz, 0.0, g)
        A[:, r, p] = A[:, p, r] = np.where(rot, c * arp - s * arq, arp)
        A[:, r, q] = A[:, q, r] = np.where(rot, s * arp + c * arq, arq)
        vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
        V[:, :, p] = np.where(rot[:, None], c[:, None] * vp - s[:, None] * vq, vp)
        V[:, :, q] = np.where(rot[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    return nz


def jacobi3(S):
    """(w [m, 3] ascending, V [m, 3, 3] with V[:, :, c] the eigenvector of w[:, c], sweeps [m]) of the symmetric 3x3 S [m, 6] by cyclic
    Jacobi: pivots (0, 1), (0, 2), (1, 2) per sweep; a zero pivot is skipped, one with |a_pp| + |g| == |a_pp| and |a_qq| + |g| == |a_qq| is
    set to zero without a rotation; else theta = (a_qq - a_pp) / (2 g), t = 1 / (|theta| + sqrt(theta theta + 1)) (1 / (|theta| + |theta|)
    above 2^500), negated for theta < 0, c = 1 / sqrt(t t + 1), s = t c, h = t g; a_pp -= h, a_qq += h, (a_rp, a_rq) = (c a_rp - s a_rq,
    s a_rp + c a_rq), columns (v_p, v_q) = (c v_p - s v_q, s v_p + c v_q).  A row stops at its first sweep that finds the three
    off-diagonals zero, or after MAX_SWEEPS; ``sweeps`` counts the others.  Equal eigenvalues keep the order of their columns."""
    S = np.asarray(S, np.float64).reshape(-1, 6)
    m = len(S)
    A = np.empty((m, 3, 3))
    for s, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        A[:, a, b] = A[:, b, a] = S[:, s]
    V = np.broadcast_to(np.eye(3), (m, 3, 3)).copy()
    sweeps = np.zeros(m, np.int64)
    for _ in range(MAX_SWEEPS):
        any_ = _pivot(A, V, 0, 1)
        any_ = _pivot(A, V, 0, 2) | any_
        any_ = _pivot(A, V, 1, 2) | any_
        if not any_.any():
            break
        sweeps += any_
    l = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1)
    o = np.broadcast_to(np.arange(3), (m, 3)).copy()
    for i, j in ((0, 1), (1, 2), (0, 1)):
        with np.errstate(invalid="ignore"):
            sw = l[:, j] < l[:, i]
        l[:, i], l[:, j] = np.where(sw, l[:, j], l[:, i]), np.where(sw, l[:, i], l[:, j])
        o[:, i], o[:, j] = np.where(sw, o[:, j], o[:, i]), np.where(sw, o[:, i], o[:, j])
    V = np.take_along_axis(V, o[:, None, :], axis=2)
    return l, V, sweeps


def normal_of(count, w, v, origin=None, viewpoint=None):
    """(normals fp32 [m, 3], valid bool [m]) from eigenvalues w [m, 3] and the smallest one's eigenvector v [m, 3]"""
    count = np.asarray(count, np.int64)
    with np.errstate(all="ignore"):
        valid = (count >= 3) & np.isfinite(w).all(1) & (w[:, 1] > 0.0)
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        n = v / length[:, None]
        if viewpoint is None:
            ax = np.zeros(len(n), np.int64)
            ax = np.where(np.abs(n[:, 1]) > np.abs(n[:, 0]), 1, ax)
            ax = np.where(np.abs(n[:, 2]) > np.abs(np.take_along_axis(n, ax[:, None], 1)[:, 0]), 2, ax)
            flip = np.take_along_axis(n, ax[:, None], 1)[:, 0] < 0.0
        else:
            e = (np.broadcast_to(np.asarray(viewpoint, np.float32).reshape(-1, 3), n.shape).astype(np.float64)
                 - np.asarray(origin, np.float32).astype(np.float64))
            flip = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2] < 0.0
        n = np.where(flip[:, None], -n, n).astype(np.float32)
    n[~valid] = 0.0
    return n, valid


def normals_from(points, idx, count, origin, viewpoint=None, scatter_of=scatter):
    """nsa_cloud_normals: dict(normals fp32 [m, 3], eigenvalues float64 [m, 3], valid bool [m], sweeps [m])"""
    count = np.asarray(count, np.int64)
    S, ok = scatter_of(points, idx, count)
    w, V, sweeps = jacobi3(S)
    n, valid = normal_of(np.where(ok, count, 0), w, V[:, :, 0], origin, viewpoint)
    w = np.where(np.isnan(w), NAN64, w)
    return dict(normals=n, eigenvalues=w, valid=valid, sweeps=sweeps)


def estimate_normals(points, k=30, max_dist=math.inf, viewpoint=None, queries=None, knn=knn_brute, scatter_of=scatter):
    """cloud_normals.estimate_normals(..., info=True): (normals, dict(valid, eigenvalues, variation, count, idx))"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    q = p if queries is None else np.asarray(queries, np.float32).reshape(-1, 3)
    _, idx, count = knn(q, p, k, max_dist)
    r = normals_from(p, idx, count, q, viewpoint, scatter_of)
    w = r["eigenvalues"]
    with np.errstate(all="ignore"):
        variation = w[:, 0] / ((w[:, 0] + w[:, 1]) + w[:, 2])
    return r["normals"], dict(valid=r["valid"], eigenvalues=w, variation=variation, count=count, idx=idx)


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------

def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def neighbourhoods(family, rows, rng, kmax=64):
    """(points fp32 [rows * kmax, 3], idx [rows, kmax], count [rows]): ``rows`` neighbourhoods of 3 .. kmax points each, of one family: "slab" (a
    thin slab, thickness 1e-3 .. 1e-1 of its extent), "offset" (a slab moved to coordinate 1000), "blob" (isotropic) or "lattice" (a plane
    lattice with a jitter of 1e-4), randomly rotated and rounded to fp32"""
    pts = np.zeros((rows, kmax, 3))
    count = rng.integers(3, kmax + 1, rows)
    for i in range(rows):
        if family == "lattice":
            g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2)[rng.permutation(64)[:kmax]]
            x = np.concatenate([g * 0.05, rng.normal(0, 1e-4, (kmax, 1))], 1)
        else:
            thick = 1.0 if family == "blob" else 10.0 ** rng.uniform(-3, -1)
            x = rng.normal(size=(kmax, 3)) * np.array([1.0, rng.uniform(0.3, 1.0), thick])
        x = x @ rotation(rng).T
        if family == "offset":
            x = x + 1000.0 * rotation(rng)[0]
        pts[i] = x
    points = pts.reshape(-1, 3).astype(np.float32)
    idx = np.arange(rows * kmax).reshape(rows, kmax)
    return points, idx, count


FAMILIES = ("slab", "offset", "blob", "lattice")


def knn_prefix(ref, k):
    """the answer for a smaller k from one for a larger: the order is total, so it is the first k columns"""
    dist, idx, count = ref
    return dist[:, :k].copy(), idx[:, :k].copy(), np.minimum(count, k)


def d2_fma(queries, targets):
    """MUTANT: the d2 a compiler contracts to fma(dz, dz, fma(dx, dx, dy * dy)); fp32 products are exact in float64"""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    t = np.asarray(targets, np.float32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = ((t[None, :, k] - q[:, None, k]).astype(np.float64) for k in range(3))
        s = (dx * dx + (dy * dy).astype(np.float32)).astype(np.float32)
        return (dz * dz + s).astype(np.float32)


def scatter_index_order(points, idx, count):
    """MUTANT: the neighbours summed in ascending index order instead of the query's (d2, index) order"""
    idx = np.asarray(idx, np.int64)
    live = np.arange(idx.shape[1])[None, :] < np.asarray(count)[:, None]
    return scatter(points, np.sort(np.where(live, idx, np.iinfo(np.int64).max), axis=1), count)


def uniform(n, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


def uniform_queries(n, seed=0):
    """the cloud's own points (each its own first neighbour) and 300 points of a larger box"""
    return np.concatenate([uniform(n, seed), np.random.default_rng(seed + 50).uniform(-1.3, 1.3, (300, 3)).astype(np.float32)])


def lattice_case():
    """(targets, queries): the 9x9x9 integer lattice, queried at its points and at its cell centres -- exact fp32 ties everywhere"""
    return lattice(9), np.concatenate([lattice(9), lattice(8) + np.float32(0.5)])


def lattice(n=9):
    """the n^3 integer lattice as fp32 points, x slowest"""
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def noisy_plane(n=2000, offset=0.0, seed=0, noise=2e-3):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.normal(0, noise, (n, 1))], 1) @ rotation(rng).T
    return (x + offset).astype(np.float32)


def sphere(n=2000, seed=1, radius=1.0, centre=(0.2, -0.1, 0.3)):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 3))
    return (x / np.linalg.norm(x, axis=1, keepdims=True) * radius + np.asarray(centre)).astype(np.float32)
