"""Oracle of mesh rasterisation and visibility (include/nicer_slam_amd.h Section 12) in numpy float32 and int64: every floating-point
operation an elementwise product, sum, quotient or square root rounded on its own, every coverage test exact integer arithmetic, one
candidate pixel centre at a time per face (vectorised ACROSS faces: all faces' candidate number t are evaluated together, which
changes no value).  Also the fixtures the mesh-render tests share: the analytic room of tests/tsdf_ref.py as a subdivided box mesh,
its closed-form wall and depth along a pixel ray in float64, and an occluding slab."""
import numpy as np

import tsdf_ref

F = np.float32
GUARD = F(16384.0)
FAR = F(1e30)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
N_TOTALS = 12
OK, BAD_INDEX, DEPTH, GUARD_FAIL, DEGENERATE, BACKFACE = 0, 1, 2, 3, 4, 5
ANY, ALL, FRUSTUM = 0, 1, 2


def w2c_rows(c2w):
    """camera-to-world [n, 4, 4] -> fp32 [n, 3, 4], inverted in float64 and rounded once"""
    return np.ascontiguousarray(np.linalg.inv(np.asarray(c2w, dtype=np.float64).reshape(-1, 4, 4))[:, :3, :].astype(F))


def project(M, K4, near, v):
    """Section 12 "Vertex" for v [m, 3] fp32 -> (code [m], x, y, p2 fp32 [m])"""
    with np.errstate(all="ignore"):
        v = np.asarray(v, dtype=F).reshape(-1, 3)
        p = [((M[r, 0] * v[:, 0] + M[r, 1] * v[:, 1]) + M[r, 2] * v[:, 2]) + M[r, 3] for r in range(3)]
        fx, fy, cx, cy = (F(t) for t in K4)
        code = np.zeros(len(v), dtype=np.int64)
        depth_ok = (p[2] > F(near)) & (p[2] <= FAR)
        x = (p[0] * fx) / p[2] + cx
        y = (p[1] * fy) / p[2] + cy
        guard_ok = (np.abs(x) <= GUARD) & (np.abs(y) <= GUARD)
        code[~guard_ok] = GUARD_FAIL
        code[~depth_ok] = DEPTH
        assert x.dtype == F and p[2].dtype == F
        return code, x, y, p[2]


def snap(x):
    with np.errstate(all="ignore"):
        return np.rint(np.where(np.isfinite(x), x, 0).astype(F) * F(256.0)).astype(np.int64)


def rotate_faces(faces, V):
    """(valid [F], A, B, C [F]): indices rotated so that the smallest comes first, winding kept"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < V)).all(1)
    i0, i1, i2 = f[:, 0], f[:, 1], f[:, 2]
    first = (i0 <= i1) & (i0 <= i2)
    second = ~first & (i1 <= i2)
    A = np.where(first, i0, np.where(second, i1, i2))
    B = np.where(first, i1, np.where(second, i2, i0))
    C = np.where(first, i2, np.where(second, i0, i1))
    return valid, A, B, C


def _owns(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


class Setup:
    """Section 12 "Face" for all faces in one view: code [F] and, where code == OK, the swapped integer triangle"""

    def __init__(self, verts, faces, M, K4, near, cull_backface=False):
        verts = np.asarray(verts, dtype=F).reshape(-1, 3)
        V = len(verts)
        valid, A, B, C = rotate_faces(faces, V)
        self.idx = [np.where(valid, t, 0) for t in (A, B, C)]
        n = len(valid)
        if V == 0:
            verts = np.zeros((1, 3), F)
        pr = [project(M, K4, near, verts[t]) for t in self.idx]
        code = np.zeros(n, dtype=np.int64)
        X = [snap(q[1]) for q in pr]
        Y = [snap(q[2]) for q in pr]
        with np.errstate(all="ignore"):
            iz = [F(1.0) / q[3] for q in pr]
        area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        swapped = area2 < 0
        if cull_backface:
            code[~swapped] = BACKFACE
        code[area2 == 0] = DEGENERATE
        code[(pr[0][0] == GUARD_FAIL) | (pr[1][0] == GUARD_FAIL) | (pr[2][0] == GUARD_FAIL)] = GUARD_FAIL
        code[(pr[0][0] == DEPTH) | (pr[1][0] == DEPTH) | (pr[2][0] == DEPTH)] = DEPTH
        code[~valid] = BAD_INDEX
        self.code, self.swapped = code, swapped
        self.X = [X[0], np.where(swapped, X[2], X[1]), np.where(swapped, X[1], X[2])]
        self.Y = [Y[0], np.where(swapped, Y[2], Y[1]), np.where(swapped, Y[1], Y[2])]
        self.iz = [iz[0], np.where(swapped, iz[2], iz[1]), np.where(swapped, iz[1], iz[2])]
        self.vid = [self.idx[0], np.where(swapped, self.idx[2], self.idx[1]), np.where(swapped, self.idx[1], self.idx[2])]
        self.area2 = np.abs(area2)
        self.fa = self.area2.astype(F)
        ax, bx, cx = self.X
        ay, by, cy = self.Y
        self.own = [_owns(cx - bx, cy - by), _owns(ax - cx, ay - cy), _owns(bx - ax, by - ay)]

    def box(self, H, W):
        xs, ys = np.stack(self.X), np.stack(self.Y)
        i0 = np.maximum(0, (xs.min(0) + 255) >> 8)
        i1 = np.minimum(W - 1, xs.max(0) >> 8)
        j0 = np.maximum(0, (ys.min(0) + 255) >> 8)
        j1 = np.minimum(H - 1, ys.max(0) >> 8)
        return i0, i1, j0, j1

    def pixel(self, f, i, j):
        """faces f [m] at pixel centres (i, j) [m] -> (covered [m], depth fp32 [m], (l0, l1, l2))"""
        ax, bx, cx = (t[f] for t in self.X)
        ay, by, cy = (t[f] for t in self.Y)
        px, py = 256 * np.asarray(i, dtype=np.int64), 256 * np.asarray(j, dtype=np.int64)
        w0 = (cx - bx) * (py - by) - (cy - by) * (px - bx)
        w1 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
        w2 = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        cov = (((w0 > 0) | ((w0 == 0) & self.own[0][f])) & ((w1 > 0) | ((w1 == 0) & self.own[1][f]))
               & ((w2 > 0) | ((w2 == 0) & self.own[2][f])))
        with np.errstate(all="ignore"):
            fa = self.fa[f]
            l0, l1, l2 = w0.astype(F) / fa, w1.astype(F) / fa, w2.astype(F) / fa
            invz = (l0 * self.iz[0][f] + l1 * self.iz[1][f]) + l2 * self.iz[2][f]
            depth = F(1.0) / invz
        assert depth.dtype == F
        return cov, depth, (l0, l1, l2)


def _keys(depth, ids):
    return (np.ascontiguousarray(depth, dtype=F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)


def raster(verts, faces, w2c, K, H, W, near, points=None, point_size=1, cull_backface=False, zbuf=None, totals=None):
    """-> (zbuf uint64 [n, H, W], totals uint64 [N_TOTALS]); K [n or 1, 4].  totals[7] and [8] (the large-face queue) stay 0."""
    w2c = np.asarray(w2c, dtype=F).reshape(-1, 3, 4)
    K = np.asarray(K, dtype=F).reshape(-1, 4)
    n = len(w2c)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nF = len(faces)
    if zbuf is None:
        zbuf = np.full((n, H, W), EMPTY, dtype=np.uint64)
        totals = np.zeros(N_TOTALS, dtype=np.uint64)
    for k in range(n):
        K4 = K[k if len(K) > 1 else 0]
        zb = zbuf[k].reshape(-1)
        if nF:
            s = Setup(verts, faces, w2c[k], K4, near, cull_backface)
            for c in range(6):
                totals[c] += np.uint64((s.code == c).sum())
            i0, i1, j0, j1 = s.box(H, W)
            nx, ny = i1 - i0 + 1, j1 - j0 + 1
            live = np.flatnonzero((s.code == OK) & (nx > 0) & (ny > 0))
            count = nx[live] * ny[live]
            t = 0
            while len(live):                                   # candidate number t of every face that still has one
                i, j = i0[live] + t % nx[live], j0[live] + t // nx[live]
                cov, depth, _ = s.pixel(live, i, j)
                np.minimum.at(zb, (j * W + i)[cov], _keys(depth[cov], live[cov]))
                totals[6] += np.uint64(cov.sum())
                t += 1
                keep = count > t
                live, count = live[keep], count[keep]
        if points is not None and len(points):
            code, x, y, p2 = project(w2c[k], K4, near, points)
            ok = np.flatnonzero(code == OK)
            totals[9] += np.uint64(len(ok))
            totals[10] += np.uint64(len(code) - len(ok))
            X, Y = snap(x[ok]), snap(y[ok])
            h = 128 * int(point_size)
            pi0, pi1 = np.maximum(0, (X - h + 255) >> 8), np.minimum(W - 1, ((X + h + 255) >> 8) - 1)
            pj0, pj1 = np.maximum(0, (Y - h + 255) >> 8), np.minimum(H - 1, ((Y + h + 255) >> 8) - 1)
            for dj in range(int(point_size) + 1):
                for di in range(int(point_size) + 1):
                    i, j = pi0 + di, pj0 + dj
                    cov = (i <= pi1) & (j <= pj1)
                    np.minimum.at(zb, (j * W + i)[cov], _keys(p2[ok][cov], nF + ok[cov]))
                    totals[6] += np.uint64(cov.sum())
    return zbuf, totals


def resolve(verts, faces, w2c, K, near, zbuf, colours=None, point_colour=None, palette=None, n_points=0, flip_to_camera=False):
    """-> dict(face_id int32, depth fp32 [n, H, W], normal, colour fp32 [n, H, W, 3], shade fp32 [n, H, W])"""
    w2c = np.asarray(w2c, dtype=F).reshape(-1, 3, 4)
    K = np.asarray(K, dtype=F).reshape(-1, 4)
    verts = np.asarray(verts, dtype=F).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n, H, W = zbuf.shape
    nF = len(faces)
    ids = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hit = (zbuf != EMPTY) & (ids < nF + n_points)
    out = dict(face_id=np.where(hit, ids, -1).astype(np.int32),
               depth=np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(F), F(0)).astype(F),
               normal=np.zeros((n, H, W, 3), F), colour=np.zeros((n, H, W, 3), F), shade=np.zeros((n, H, W), F))
    for k in range(n):
        K4 = K[k if len(K) > 1 else 0]
        M = w2c[k]
        pt = np.argwhere(hit[k] & (ids[k] >= nF))
        if len(pt):
            out["shade"][k, pt[:, 0], pt[:, 1]] = 1.0
            if point_colour is not None and palette is not None:
                ci = np.asarray(point_colour, dtype=np.int64)[ids[k, pt[:, 0], pt[:, 1]] - nF]
                good = (ci >= 0) & (ci < len(palette))
                out["colour"][k, pt[good, 0], pt[good, 1]] = np.asarray(palette, dtype=F).reshape(-1, 3)[ci[good]]
        px = np.argwhere(hit[k] & (ids[k] < nF))
        if not len(px):
            continue
        j, i = px[:, 0], px[:, 1]
        f = ids[k, j, i]
        s = Setup(verts, faces, M, K4, near, False)
        good = s.code[f] == OK
        cov, depth, (l0, l1, l2) = s.pixel(f, i, j)
        good &= cov
        j, i, f, l0, l1, l2 = j[good], i[good], f[good], l0[good], l1[good], l2[good]
        with np.errstate(all="ignore"):
            if colours is not None:
                col = np.asarray(colours, dtype=F).reshape(-1, 3)
                q0, q1, q2 = l0 * s.iz[0][f], l1 * s.iz[1][f], l2 * s.iz[2][f]
                invz = (q0 + q1) + q2
                cA, cB, cC = col[s.vid[0][f]], col[s.vid[1][f]], col[s.vid[2][f]]
                out["colour"][k, j, i] = ((q0[:, None] * cA + q1[:, None] * cB) + q2[:, None] * cC) / invz[:, None]
            a, b, c = verts[s.idx[0][f]], verts[s.idx[1][f]], verts[s.idx[2][f]]
            e1, e2 = b - a, c - a
            cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
            fine = (ln > 0) & (ln <= F(3.0e38))
            nrm = np.where(fine[:, None], np.stack([cx, cy, cz], -1) / ln[:, None], F(0)).astype(F)
            nc = [(M[r, 0] * nrm[:, 0] + M[r, 1] * nrm[:, 1]) + M[r, 2] * nrm[:, 2] for r in range(3)]
            dx, dy = (i.astype(F) - K4[2]) / K4[0], (j.astype(F) - K4[3]) / K4[1]
            dl = np.sqrt((dx * dx + dy * dy) + F(1.0))
            sh = np.abs(((nc[0] * dx + nc[1] * dy) + nc[2]) / dl)
            out["shade"][k, j, i] = np.where(fine, sh, F(0))
            if flip_to_camera:
                nrm = np.where((fine & ~s.swapped[f])[:, None], -nrm, nrm)
            out["normal"][k, j, i] = nrm
    return out


def vertex_seen(v, M, K4, near, H, W, zb, depth_test, rel):
    """Section 12 "Visibility" of vertices v [m, 3] in one finished view zb uint64 [H, W] -> bool [m]"""
    code, x, y, p2 = project(M, K4, near, v)
    with np.errstate(all="ignore"):
        seen = (code == OK) & (x >= 0) & (x <= F(W - 1)) & (y >= 0) & (y <= F(H - 1))
        if not depth_test:
            return seen
        xs, ys = np.where(seen, x, 0), np.where(seen, y, 0)
        i0, j0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
        i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
        top = np.maximum(np.maximum(zb[j0, i0], zb[j0, i1]), np.maximum(zb[j1, i0], zb[j1, i1])) >> np.uint64(32)
        zmax = top.astype(np.uint32).view(F)
        slack = F(1.0) + F(rel)
        return seen & ((top == np.uint64(0xFFFFFFFF)) | (p2 <= slack * zmax))


def visible(verts, faces, w2c, K, H, W, near, zbuf, mode, rel):
    """-> uint8 [F]"""
    w2c = np.asarray(w2c, dtype=F).reshape(-1, 3, 4)
    K = np.asarray(K, dtype=F).reshape(-1, 4)
    verts = np.asarray(verts, dtype=F).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < len(verts))).all(1)
    fi = np.where(valid[:, None], f, 0)
    out = np.zeros(len(f), dtype=bool)
    for k in range(len(w2c)):
        K4 = K[k if len(K) > 1 else 0]
        seen = vertex_seen(verts if len(verts) else np.zeros((1, 3), F), w2c[k], K4, near, H, W,
                           None if zbuf is None else zbuf[k], mode != FRUSTUM, rel)
        s = seen[fi]
        out |= valid & (s.all(1) if mode == ALL else s.any(1))
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------- fixtures
def room_mesh(n=4, half=tsdf_ref.ROOM_HALF):
    """The room of tsdf_ref as a box mesh with each wall split n x n: dict(verts fp32 [6 (n + 1)^2, 3], faces int32 [12 n^2, 3],
    colors fp32).  Wall w = 2 * axis + (1 if on the positive side) owns faces [2 n^2 w, 2 n^2 (w + 1)); walls share no vertices."""
    verts, faces = [], []
    h = np.asarray(half, dtype=np.float64)
    for w in range(6):
        a, side = w // 2, (1.0 if w % 2 else -1.0)
        b, c = (a + 1) % 3, (a + 2) % 3
        base = len(verts)
        for p in range(n + 1):
            for q in range(n + 1):
                v = np.zeros(3)
                v[a], v[b], v[c] = side * h[a], h[b] * (2.0 * p / n - 1.0), h[c] * (2.0 * q / n - 1.0)
                verts.append(v)
        for p in range(n):
            for q in range(n):
                i00, i01, i10, i11 = (base + p * (n + 1) + q, base + p * (n + 1) + q + 1, base + (p + 1) * (n + 1) + q,
                                      base + (p + 1) * (n + 1) + q + 1)
                faces += [(i00, i10, i11), (i00, i11, i01)] if side < 0 else [(i00, i11, i10), (i00, i01, i11)]
    verts = np.asarray(verts, dtype=F)
    colors = (0.5 + 0.5 * np.sin(verts.astype(np.float64) * [3.0, 5.0, 7.0] + [0.1, 0.2, 0.3])).astype(F)
    return dict(verts=verts, faces=np.asarray(faces, dtype=np.int32), colors=colors)


def wall_of_face(face_id, n):
    return np.where(face_id >= 0, face_id // (2 * n * n), -1)


def room_hit(c2w, K4, x, y, half=tsdf_ref.ROOM_HALF):
    """Closed form in float64 for a camera INSIDE the room: the ray through pixel coordinates (x, y) (arrays) leaves the box through
    wall w at z-depth d -> (w, d, g) with g = |d(1/z)/dx| + |d(1/z)/dy| of that wall's plane on the screen (per pixel)."""
    P = np.asarray(c2w, dtype=np.float64)
    fx, fy, cx, cy = (float(t) for t in K4)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d_cam = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1)
    d_w = d_cam @ P[:3, :3].T
    o = P[:3, 3]
    h = np.asarray(half, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = np.where(d_w > 0, (h - o) / d_w, np.where(d_w < 0, (-h - o) / d_w, np.inf))       # z-depth at which each slab is left
    a = t.argmin(-1)
    d = t.min(-1)
    w = 2 * a + (np.take_along_axis(d_w, a[..., None], -1)[..., 0] > 0)
    # the wall's plane: n_w . X = h_a (n_w = +-e_a); in the camera frame 1/z = n_c . (dx, dy, 1) / (h_a -+ o_a)
    sign = np.where(w % 2 == 1, 1.0, -1.0)
    n_c = sign[..., None] * P[:3, :3][a]                  # row a of R_c2w = e_a in the camera frame
    dist = h[a] - sign * o[a]
    g = np.abs(n_c[..., 0] / (fx * dist)) + np.abs(n_c[..., 1] / (fy * dist))
    return w, d, g


def slab_mesh(lo, hi):
    """an axis-aligned box [lo, hi] as 12 triangles"""
    lo, hi = np.asarray(lo, dtype=F), np.asarray(hi, dtype=F)
    m = tsdf_ref.box_mesh((1.0, 1.0, 1.0))
    verts = (lo + (m["verts"] * F(0.5) + F(0.5)) * (hi - lo)).astype(F)
    return dict(verts=verts, faces=m["faces"])


def merge(*meshes):
    verts, faces, off = [], [], 0
    for m in meshes:
        verts.append(np.asarray(m["verts"], dtype=F))
        faces.append(np.asarray(m["faces"], dtype=np.int32) + off)
        off += len(m["verts"])
    return dict(verts=np.concatenate(verts), faces=np.concatenate(faces).astype(np.int32))


def snap_bound_units(verts, M, K4):
    """The header's bound on |X - 256 x_exact| (and the same for Y), in units of 1/256 pixel, per vertex (float64), with a 1 %
    allowance for the second-order terms."""
    v = np.asarray(verts, dtype=np.float64)
    Md = np.asarray(M, dtype=np.float64)
    fx, fy, cx, cy = (float(t) for t in K4)
    u = 2.0 ** -24
    m = [np.abs(Md[r, :3] * v).sum(1) + abs(Md[r, 3]) for r in range(3)]
    p = [v @ Md[r, :3] + Md[r, 3] for r in range(3)]
    out = []
    for r, f, c in ((0, fx, cx), (1, fy, cy)):
        xe = p[r] * f / p[2] + c
        out.append(0.5 + 1.01 * 256.0 * u * (4 * f * m[r] / p[2] + np.abs(xe - c) * (2 + 4 * m[2] / p[2]) + np.abs(xe)))
    return out, (p[0] * fx / p[2] + cx, p[1] * fy / p[2] + cy)


def depth_term_rel(verts, M):
    """Relative error of a vertex's fp32 p_2 against the exact one, per vertex (float64): four roundings, each at most
    u = 2^-24 of m_2 = |R_20 v_x| + |R_21 v_y| + |R_22 v_z| + |t_2|, so 4 u m_2 / |p_2| (1 % allowed for the second order)."""
    v = np.asarray(verts, dtype=np.float64)
    Md = np.asarray(M, dtype=np.float64)
    m2 = np.abs(Md[2, :3] * v).sum(1) + abs(Md[2, 3])
    p2 = v @ Md[2, :3] + Md[2, 3]
    with np.errstate(all="ignore"):
        return 1.01 * 4 * 2.0 ** -24 * m2 / np.abs(p2)

