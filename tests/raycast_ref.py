"""numpy float64 oracle of the ray cast against a triangle mesh (include/nicer_slam_amd.h Section 17, csrc/mesh_raycast.hip): the
per-face watertight test with and without its box clause, the brute force over the usable faces, the tree with the header's layout
and the ordered walk with its counts; plus the rays and meshes the tests share.  numpy rounds every elementwise operation on its own,
which is the contract: t, the face and the barycentrics carry the kernel's bits."""
import numpy as np

import p2m_ref as P

MAX_LEVEL = 10
PAD_REL = np.float32(2.0 ** -20)
ANY_HIT, CULL_BACK, CULL_FRONT = 1, 2, 4


def level_of(n):
    L = 0
    while L < MAX_LEVEL and 8 * 4 ** L < n:
        L += 1
    return L


def max_nodes(F):
    return sum(min(8 ** l, F) for l in range(level_of(F) + 1))


def workspace_bound(F):
    """the header's byte count without the rounding of its 12 arrays to 256 bytes"""
    return 256 + 24 * F + 4 + 24 * F + 68 * max_nodes(F) + (1 << 18)


def _morton(cell, L):
    key = np.zeros(cell.shape[0], np.int64)
    for bit in range(L):
        for k in range(3):
            key |= ((cell[:, k] >> bit) & 1) << (3 * bit + (2 - k))
    return key


def face_boxes(a, b, c):
    """[n, 6] float32: the padded boxes of faces with fp32 vertices a, b, c [n, 3], every step in fp32"""
    a, b, c = (np.asarray(x, np.float32) for x in (a, b, c))
    s = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.abs(c)).max(1)
    pad = (s * PAD_REL).astype(np.float32)[:, None]
    lo = (np.minimum(np.minimum(a, b), c) - pad).astype(np.float32)
    hi = (np.maximum(np.maximum(a, b), c) + pad).astype(np.float32)
    with np.errstate(over="ignore"):
        return np.concatenate([np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))], 1).astype(np.float32)


class Tree:
    """the tree of Section 17 over (verts, faces): the sorted usable faces (``face`` their indices, ``a``, ``b``, ``c`` their float64
    vertices, ``fbox`` their boxes) and the nodes in pre-order: level, begin, end, skip, leaf, lo, hi, child [K, 8] (0 = none)"""

    def __init__(self, verts, faces):
        v32 = np.asarray(verts, np.float32)
        v = v32.astype(np.float64)
        f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
        use = np.nonzero(P.face_causes(verts, f) == 0)[0]
        self.F, self.n_usable = f.shape[0], use.size
        self.L = L = level_of(use.size)
        self.n_nodes = 0
        self.face = use
        self.a = self.b = self.c = np.zeros((0, 3))
        self.fbox = np.zeros((0, 6))
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
        self.a, self.b, self.c = a[order], b[order], c[order]
        fs = f[self.face]
        self.fbox = face_boxes(v32[fs[:, 0]], v32[fs[:, 1]], v32[fs[:, 2]]).astype(np.float64)
        n = use.size
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
        self.child = np.zeros((K, 8), np.int64)
        prefix = [self.key >> (3 * (L - l)) for l in range(L + 1)]
        for i in np.nonzero(h[:n])[0]:
            lmin = L + 1 - h[i]
            for l in range(lmin, L + 1):
                k = base[i] + (l - lmin)
                e = int(np.searchsorted(prefix[l], prefix[l][i], side="right"))
                self.level[k], self.begin[k], self.end[k], self.skip[k] = l, i, e, base[e]
        by_start = {(int(self.level[k]), int(self.begin[k])): k for k in range(K)}
        for k in range(1, K):
            l, i = int(self.level[k]), int(self.begin[k])
            first = int(np.searchsorted(prefix[l - 1], prefix[l - 1][i], side="left"))
            self.child[by_start[(l - 1, first)], int(prefix[l][i]) & 7] = k
        self.leaf = self.level == L
        self.lo, self.hi = np.zeros((K, 3)), np.zeros((K, 3))
        for l in range(L + 1):
            ks = np.nonzero(self.level == l)[0]                      # in pre-order, so their ranges ascend and tile [0, n)
            self.lo[ks] = np.minimum.reduceat(self.fbox[:, :3], self.begin[ks], axis=0)
            self.hi[ks] = np.maximum.reduceat(self.fbox[:, 3:], self.begin[ks], axis=0)


def _tree(mesh_or_tree, faces=None):
    return mesh_or_tree if isinstance(mesh_or_tree, Tree) else Tree(mesh_or_tree, faces)


class Rays:
    """the per-ray quantities of the header, for fp32 origins and directions [m, 3]"""

    def __init__(self, origins, dirs, tmin=0.0, tmax=np.inf):
        o = np.asarray(origins, np.float32).astype(np.float64).reshape(-1, 3)
        d = np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
        assert o.shape == d.shape
        self.m = o.shape[0]
        self.valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
        o, d = np.where(self.valid[:, None], o, 0.0), np.where(self.valid[:, None], d, 1.0)
        self.o, self.d = o, d
        ad = np.abs(d)
        kz = np.zeros(self.m, np.int64)
        kz = np.where(ad[:, 1] > ad[:, 0], 1, kz)
        kz = np.where(ad[:, 2] > np.take_along_axis(ad, kz[:, None], 1)[:, 0], 2, kz)
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        dz = np.take_along_axis(d, kz[:, None], 1)[:, 0]
        kx, ky = np.where(dz < 0, ky, kx), np.where(dz < 0, kx, ky)
        self.kx, self.ky, self.kz = kx, ky, kz
        self.Sx = np.take_along_axis(d, kx[:, None], 1)[:, 0] / dz
        self.Sy = np.take_along_axis(d, ky[:, None], 1)[:, 0] / dz
        self.Sz = 1.0 / dz
        with np.errstate(divide="ignore"):
            self.inv = 1.0 / d
        self.zero = d == 0
        self.oct = (d[:, 0] < 0) * 4 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 1
        self.tmin, self.tmax = float(tmin), float(tmax)


def slab(rays, idx, lo, hi):
    """(ok, enter, exit) of rays[idx] against boxes lo, hi [len(idx), 3] (or broadcastable [len(idx), n, 3] with idx[:, None])"""
    o, inv, zero = rays.o[idx], rays.inv[idx], rays.zero[idx]
    with np.errstate(all="ignore"):
        x, y = (lo - o) * inv, (hi - o) * inv
    near = np.where(zero, -np.inf, np.minimum(x, y))
    far = np.where(zero, np.inf, np.maximum(x, y))
    inside = np.where(zero, (lo <= o) & (o <= hi), True).all(-1)
    enter = np.maximum(np.maximum(np.maximum(rays.tmin, near[..., 0]), near[..., 1]), near[..., 2])
    exit_ = np.minimum(np.minimum(np.minimum(rays.tmax, far[..., 0]), far[..., 1]), far[..., 2])
    return inside & (enter <= exit_), enter, exit_


def woop(rays, idx, a, b, c, flags=0):
    """(pass, t, U, V, W, det) of the face test without its box clause: rays[idx] against faces a, b, c (same leading shape as idx)"""
    o = rays.o[idx]
    kx, ky, kz = rays.kx[idx][..., None], rays.ky[idx][..., None], rays.kz[idx][..., None]
    Sx, Sy, Sz = rays.Sx[idx], rays.Sy[idx], rays.Sz[idx]
    pick = lambda X, k: np.take_along_axis(X, np.broadcast_to(k, X.shape[:-1] + (1,)), -1)[..., 0]
    with np.errstate(all="ignore"):
        A, B, C = a - o, b - o, c - o
        Az, Bz, Cz = pick(A, kz), pick(B, kz), pick(C, kz)
        Ax, Ay = pick(A, kx) - Sx * Az, pick(A, ky) - Sy * Az
        Bx, By = pick(B, kx) - Sx * Bz, pick(B, ky) - Sy * Bz
        Cx, Cy = pick(C, kx) - Sx * Cz, pick(C, ky) - Sy * Cz
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        ok = ~(((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0)))
        det = (U + V) + W
        ok &= det != 0
        if flags & CULL_BACK:
            ok &= ~(det < 0)
        if flags & CULL_FRONT:
            ok &= ~(det > 0)
        T = (U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)
        t = T / det
    return ok, t, U, V, W, det


def _answer(rays, best_t, best_face, uvw, det):
    hit = rays.valid & (best_face >= 0)
    with np.errstate(all="ignore"):
        bary = np.where(hit[:, None], uvw / det[:, None], np.nan)
    t = np.where(rays.valid, np.where(hit, best_t, np.inf), np.nan)
    return t, np.where(hit, best_face, -1).astype(np.int64), bary


def brute(origins, dirs, tree, tmin=0.0, tmax=np.inf, flags=0, box=True, pairs=200_000):
    """dict(t, face, bary, hit): the best hit over every usable face; ``box=False`` drops the box clause of the face test (t in
    [tmin, tmax] alone) -- the two must agree on a sane mesh"""
    rays = Rays(origins, dirs, tmin, tmax)
    M, n = rays.m, tree.n_usable
    best_t, best_face = np.full(M, np.inf), np.full(M, -1, np.int64)
    uvw, det = np.zeros((M, 3)), np.ones(M)
    step = max(1, pairs // max(n, 1))
    for lo in range(0, M if n else 0, step):
        idx = np.arange(lo, min(lo + step, M))[:, None]
        ok, t, U, V, W, D = woop(rays, idx, tree.a[None], tree.b[None], tree.c[None], flags)
        if box:
            inside, enter, exit_ = slab(rays, idx, tree.fbox[None, :, :3], tree.fbox[None, :, 3:])
            ok &= inside & (enter <= t) & (t <= exit_)
        else:
            ok &= (rays.tmin <= t) & (t <= rays.tmax)
        ok &= t < np.inf
        tt = np.where(ok, t, np.inf)
        tb = tt.min(1)
        cand = np.where(ok & (tt == tb[:, None]), tree.face[None], np.iinfo(np.int64).max)
        pos = cand.argmin(1)
        got = ok.any(1)
        r = idx[:, 0]
        best_t[r] = np.where(got, tb, np.inf)
        best_face[r] = np.where(got, tree.face[pos], -1)
        take = lambda X: X[np.arange(len(r)), pos]
        uvw[r] = np.stack([take(U), take(V), take(W)], 1)
        det[r] = take(D)
    t, face, bary = _answer(rays, best_t, best_face, uvw, det)
    return dict(t=t, face=face, bary=bary, hit=face >= 0)


def walk(origins, dirs, tree, tmin=0.0, tmax=np.inf, flags=0):
    """dict(t, face, bary, hit, nodes, tested): the ordered walk of every ray (in lockstep, one node per ray and round)"""
    rays = Rays(origins, dirs, tmin, tmax)
    M = rays.m
    any_hit = bool(flags & ANY_HIT)
    best_t, best_face = np.full(M, np.inf), np.full(M, -1, np.int64)
    uvw, det = np.zeros((M, 3)), np.ones(M)
    nn, nt = np.zeros(M, np.int64), np.zeros(M, np.int64)
    cur, lev = np.zeros(M, np.int64), np.zeros(M, np.int64)
    path, rank = np.zeros((M, MAX_LEVEL + 1), np.int64), np.zeros((M, MAX_LEVEL + 1), np.int64)
    active = rays.valid & (tree.n_nodes > 0)

    def try_faces(idx, pos):
        ok, enter, exit_ = slab(rays, idx, tree.fbox[pos, :3], tree.fbox[pos, 3:])
        run = ok if any_hit else ok & ~(enter > best_t[idx])
        idx, pos, enter, exit_ = idx[run], pos[run], enter[run], exit_[run]
        nt[idx] += 1
        ok, t, U, V, W, D = woop(rays, idx, tree.a[pos], tree.b[pos], tree.c[pos], flags)
        ok &= (enter <= t) & (t <= exit_)
        g = tree.face[pos]
        ok &= (t < best_t[idx]) | ((t == best_t[idx]) & (g < best_face[idx]))
        w = idx[ok]
        best_t[w], best_face[w], det[w] = t[ok], g[ok], D[ok]
        uvw[w] = np.stack([U[ok], V[ok], W[ok]], 1)
        return w

    while active.any():
        idx = np.nonzero(active)[0]
        n = cur[idx]
        nn[idx] += 1
        ok, enter, _ = slab(rays, idx, tree.lo[n], tree.hi[n])
        go = ok if any_hit else ok & ~(enter > best_t[idx])
        leaf = go & tree.leaf[n]
        il, nl = idx[leaf], n[leaf]
        count = tree.end[nl] - tree.begin[nl]
        alive = np.ones(il.size, bool)
        for s in range(int(count.max()) if count.size else 0):
            sel = alive & (count > s)
            won = try_faces(il[sel], tree.begin[nl[sel]] + s)
            if any_hit and won.size:
                alive &= ~np.isin(il, won)
                active[won] = False
        down = go & ~tree.leaf[n]
        idn = idx[down]
        path[idn, lev[idn]] = n[down]
        rank[idn, lev[idn]] = 0
        lev[idx[~down]] -= 1
        pending = active.copy()
        pending[~np.isin(np.arange(M), idx)] = False
        while True:
            p = np.nonzero(pending)[0]
            if p.size == 0:
                break
            over = lev[p] < 0
            active[p[over]] = False
            pending[p[over]] = False
            p = p[~over]
            r = rank[p, lev[p]]
            up = r >= 8
            lev[p[up]] -= 1
            p, r = p[~up], r[~up]
            c = tree.child[path[p, lev[p]], r ^ rays.oct[p]]
            rank[p, lev[p]] = r + 1
            got = c != 0
            cur[p[got]] = c[got]
            lev[p[got]] += 1
            pending[p[got]] = False
    t, face, bary = _answer(rays, best_t, best_face, uvw, det)
    nn[~rays.valid] = 0
    return dict(t=t, face=face, bary=bary, hit=face >= 0, nodes=nn, tested=nt)


# ---- shared rays and meshes -------------------------------------------------------------------------------------------------------

def camera_rays(c2w, intrinsics, size, pixels=None):
    """(origins, dirs) fp32 [H * W, 3] (or [k, 3] for ``pixels`` [k, 2] = (column, row)): nicer_slam_amd.mesh_raycast.camera_rays in
    numpy: d = R ((u - cx) / fx, (v - cy) / fy, 1) formed in float64 and rounded to fp32"""
    c2w = np.asarray(c2w, np.float64).reshape(4, 4)
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    if pixels is None:
        H, W = size
        v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        u, v = u.reshape(-1), v.reshape(-1)
    else:
        px = np.asarray(pixels, np.float64).reshape(-1, 2)
        u, v = px[:, 0], px[:, 1]
    x, y = (u - cx) / fx, (v - cy) / fy
    R = c2w[:3, :3]
    d = np.stack([(R[k, 0] * x + R[k, 1] * y) + R[k, 2] for k in range(3)], 1)
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    return o.astype(np.float32), d.astype(np.float32)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera-to-world [4, 4]: x right, y down, z forward"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


def sphere_rays(n=513, seed=0, r=3.0, spread=0.6):
    """n rays from the sphere of radius r about the origin aimed at points within ``spread`` of it: most hit a unit-sized mesh"""
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((n, 3))
    o *= r / np.linalg.norm(o, axis=1, keepdims=True)
    target = rng.uniform(-spread, spread, (n, 3))
    return o.astype(np.float32), (target - o).astype(np.float32)


def watertight_rays(verts, faces, n=6000, seed=0, dist=1.0, max_deg=15.0):
    """n rays aimed from outside at fp32 vertices, edge midpoints and random edge points of a star-shaped mesh about the origin,
    from within ``max_deg`` of the outward direction, starting ``dist`` (about) from the target.  -> (origins, dirs, targets)"""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)
    f = f[P.face_causes(verts, f) == 0]
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    k = n // 3
    tv = v[rng.integers(0, v.shape[0], k)]
    em = e[rng.integers(0, e.shape[0], k)]
    tm = (0.5 * (v[em[:, 0]] + v[em[:, 1]])).astype(np.float32).astype(np.float64)
    er = e[rng.integers(0, e.shape[0], n - 2 * k)]
    s = rng.uniform(0, 1, (n - 2 * k, 1))
    tr = (v[er[:, 0]] * (1 - s) + v[er[:, 1]] * s).astype(np.float32).astype(np.float64)
    target = np.concatenate([tv, tm, tr])
    out = target / np.linalg.norm(target, axis=1, keepdims=True)
    side = np.cross(out, rng.standard_normal(out.shape))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    ang = np.radians(rng.uniform(0, max_deg, (n, 1)))
    back = np.cos(ang) * out + np.sin(ang) * side
    o = (target + dist * back).astype(np.float32)
    d = (target - o.astype(np.float64)).astype(np.float32)
    return o, d, target


def welded_latlong_sphere(n_lat=24, n_lon=48):
    """P.latlong_sphere with one vertex per position.  P.latlong_sphere lists the longitude seam twice, and the column at 2 pi has
    y = sin(2 pi) = -1.2e-16 r where the column at 0 has y = 0: two fp32 positions, a crack 1e-16 wide that a ray aimed exactly
    at a seam vertex can pass through.  Section 17 promises watertightness for faces that share fp32 coordinates; this is the
    sphere that does.  Vertices within 2^-20 of each other become the first of them; the face list is kept."""
    v, f, _ = P.latlong_sphere(n_lat, n_lon)
    _, first, inverse = np.unique(np.round(v.astype(np.float64) * 2.0 ** 20), axis=0, return_index=True, return_inverse=True)
    return v, first[inverse.reshape(-1)][f].astype(np.int32)


def coincident_centroids(k=40):
    """k nested triangles of growing size about one centroid, a little apart in z: one leaf at L >= 1, every box inside the next"""
    ang = np.array([0.3, 0.3 + 2.0943951023931953, 0.3 + 4.1887902047863905])[None]
    r = (0.2 + 0.02 * np.arange(k))[:, None]
    z = np.repeat(np.linspace(0.0, 1e-4, k), 3)
    v = np.stack([(r * np.cos(ang)).reshape(-1), (r * np.sin(ang)).reshape(-1), z], 1).astype(np.float32)
    return v, np.arange(3 * k, dtype=np.int32).reshape(-1, 3)
