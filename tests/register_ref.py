"""numpy statement of point-to-plane registration (include/nicer_slam_amd.h Section 27, csrc/mesh_register.hip,
nicer_slam_amd/mesh_register.py) for the tests: the rows and their weights, the order of the thirty sums, the 6x6 LDL^T, the
update and the loop.  numpy rounds every elementwise operation on its own and never fuses a multiply with an add, which is the
contract; the host step is plain Python float arithmetic.  Correspondences come from eval_ref.nn_brute and p2m_ref.closest_brute.

The order of a sum over n terms, a function of n alone:
  1. tiles of 4096 consecutive terms, the last one padded with +0.0;
  2. lane l of 256 adds the terms l, l + 256, ... of its tile in ascending order onto +0.0 (16 additions);
  3. a binary tree over the 256 lanes, s[i] = s[2 i] + s[2 i + 1], eight levels;
  4. while more than one value is left: groups of 256 consecutive values, the last padded with +0.0, through the tree of 3."""
import math

import numpy as np

import eval_ref as E
import p2m_ref as P

TILE, LANES = 4096, 256
KERNELS = ("l2", "huber", "tukey")


def parse_kernel(kernel):
    """(name, k) of "l2" | ("huber", k) | ("tukey", k)"""
    if kernel == "l2":
        return "l2", 0.0
    name, k = kernel
    assert name in ("huber", "tukey") and k > 0
    return name, float(k)


# ---- the order ------------------------------------------------------------------------------------------------------------------

def _tree(s):
    """[..., 256, C] -> [..., C]"""
    while s.shape[-2] > 1:
        s = s[..., 0::2, :] + s[..., 1::2, :]
    return s[..., 0, :]


def ordered_sum(terms):
    """terms [n] or [n, C] float64 -> the sum(s) in the stated order, float64 scalar or [C]"""
    t = np.asarray(terms, np.float64)
    flat = t.ndim == 1
    t = t.reshape(len(t), -1)
    n, C = t.shape
    tiles = max(1, -(-n // TILE))
    pad = np.zeros((tiles * TILE, C))
    pad[:n] = t
    rows = pad.reshape(tiles, TILE // LANES, LANES, C)
    acc = np.zeros((tiles, LANES, C))
    with np.errstate(all="ignore"):
        for j in range(TILE // LANES):
            acc = acc + rows[:, j]
        vals = _tree(acc)                                   # [tiles, C]
        while len(vals) > 1:
            groups = -(-len(vals) // LANES)
            pad = np.zeros((groups * LANES, C))
            pad[:len(vals)] = vals
            vals = _tree(pad.reshape(groups, LANES, C))
    return vals[0, 0] if flat else vals[0]


def path_additions(n):
    """the number of additions on the longest path from a term to the total: 16 in the lane, 8 per tree"""
    tiles = max(1, -(-n // TILE))
    m = TILE // LANES + 8
    while tiles > 1:
        tiles = -(-tiles // LANES)
        m += 8
    return m


# ---- the rows -------------------------------------------------------------------------------------------------------------------

def face_unit_normals(verts, faces):
    """[F, 3] float64: c / sqrt((c_x c_x + c_y c_y) + c_z c_z), c = ab x ac from the fp32 vertices; NaN for a face without area or
    with an index outside [0, V)"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    fc = np.where(ok[:, None], f, 0)
    a, b, c = v[fc[:, 0]], v[fc[:, 1]], v[fc[:, 2]]
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        cx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        cy = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        cz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
        length = np.sqrt((cx * cx + cy * cy) + cz * cz)
        n = np.stack([cx / length, cy / length, cz / length], -1)
    n[~ok] = np.nan
    return n


def weights(r, kernel):
    name, k = parse_kernel(kernel)
    with np.errstate(all="ignore"):
        ar = np.abs(r)
        if name == "huber":
            return np.where(ar <= k, 1.0, k / ar)
        if name == "tukey":
            u = r / k
            v = 1.0 - u * u
            return np.where(ar <= k, v * v, 0.0)
    return np.ones_like(r)


def residuals(p, q, nrm):
    d = p - q
    return (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]


def row_terms(p, q, nrm, dd, corr, kernel, residual=residuals):
    """(terms [n, 30], used [n]) of rows p [n, 3] with correspondences q, normals nrm (float64), squared distances dd and the mask corr.
    ``residual``: a test puts a mutant in its place"""
    with np.errstate(all="ignore"):
        used = corr & np.isfinite(nrm).all(1) & ~(nrm == 0).all(1)
        r = residual(p, q, nrm)
        J = np.stack([p[:, 1] * nrm[:, 2] - p[:, 2] * nrm[:, 1], p[:, 2] * nrm[:, 0] - p[:, 0] * nrm[:, 2],
                      p[:, 0] * nrm[:, 1] - p[:, 1] * nrm[:, 0], nrm[:, 0], nrm[:, 1], nrm[:, 2]], -1)
        w = weights(r, kernel)
        g = w[:, None] * J
        cols = [g[:, i] * J[:, j] for i in range(6) for j in range(i, 6)]
        cols += [g[:, i] * r for i in range(6)]
        cols += [r * r, (w * r) * r]
        t = np.stack(cols, -1)
    t = np.where(used[:, None], t, 0.0)
    return np.concatenate([t, np.where(corr, dd, 0.0)[:, None]], 1), used


def cloud_rows(cur, idx, dist, targets, normals):
    """(p, q, nrm, dd, corr) of cloud mode"""
    cur = np.asarray(cur, np.float64)
    idx = np.asarray(idx).astype(np.int64)
    t = np.asarray(targets, np.float32).astype(np.float64)
    nn = np.asarray(normals, np.float32).astype(np.float64)
    corr = (idx >= 0) & (idx < len(t))
    safe = np.where(corr, idx, 0)
    d = np.asarray(dist, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return cur, t[safe], nn[safe], d * d, corr


def surface_rows(cur, face_idx, d2, closest, verts, faces):
    """(p, q, nrm, dd, corr) of surface mode"""
    cur = np.asarray(cur, np.float64)
    face = np.asarray(face_idx).astype(np.int64)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    corr = (face >= 0) & (face < len(f))
    safe = np.where(corr, face, 0)
    corr = corr & ((f[safe] >= 0) & (f[safe] < len(verts))).all(1)
    return cur, np.asarray(closest, np.float32).astype(np.float64), face_unit_normals(verts, f)[safe], np.asarray(d2, np.float64), corr


def system_from_rows(p, q, nrm, dd, corr, kernel, residual=residuals, reduce=ordered_sum):
    """dict(sums [30], k_corr, k_used, A [6, 6], b [6]); ``reduce``: a test puts a mutant in its place"""
    t, used = row_terms(p, q, nrm, dd, corr, kernel, residual)
    S = np.asarray(reduce(t), np.float64)
    A = np.zeros((6, 6))
    s = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = S[s]
            s += 1
    return dict(sums=S, k_corr=int(corr.sum()), k_used=int(used.sum()), A=A, b=-S[21:27], terms=t)


def plane_system(cur, kernel="l2", idx=None, dist=None, targets=None, normals=None, face_idx=None, d2=None, closest=None, verts=None,
                 faces=None):
    if idx is not None:
        return system_from_rows(*cloud_rows(cur, idx, dist, targets, normals), kernel)
    return system_from_rows(*surface_rows(cur, face_idx, d2, closest, verts, faces), kernel)


# ---- the host step --------------------------------------------------------------------------------------------------------------

def ldlt_solve(A, b):
    """x of A x = b by LDL^T without pivoting, or None when a pivot is not > 2^-40 A_jj (degenerate).  Column by column: v_k = L_jk D_k,
    D_j = A_jj - sum_k L_jk v_k and L_ij = (A_ij - sum_k L_ik v_k) / D_j, each sum subtracted term by term for k ascending; then
    L y = b forwards, z = y / D, L^T x = z backwards with k ascending in every row."""
    A = [[float(A[i][j]) for j in range(6)] for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        v = [L[j][k] * D[k] for k in range(j)]
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * v[k]
        if not d > 2.0 ** -40 * A[j][j]:
            return None
        D[j] = d
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * v[k]
            L[i][j] = s / d
    y = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    z = [y[i] / D[i] for i in range(6)]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = z[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x


def update_matrix(x):
    """open3d's TransformVector6dToMatrix4d: R = Rz(x_2) Ry(x_1) Rx(x_0), t = x_3..5"""
    ca, sa, cb, sb, cc, sc = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    return np.array([[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, x[3]],
                     [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def matmul4(U, T):
    """U T with out_ij = ((U_i0 T_0j + U_i1 T_1j) + U_i2 T_2j) + U_i3 T_3j"""
    return ((U[:, 0:1] * T[0] + U[:, 1:2] * T[1]) + U[:, 2:3] * T[2]) + U[:, 3:4] * T[3]


# ---- the loop -------------------------------------------------------------------------------------------------------------------

def icp_point_to_plane(source, target, normals=None, max_corr=0.1, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, kernel="l2"):
    """``target``: fp32 points [m, 3] with ``normals`` (cloud mode) or (verts, faces) (surface mode)"""
    src = np.asarray(source, np.float32).astype(np.float64)
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    cur = E.transform(src, T)
    if normals is not None:
        tgt, nrm = np.asarray(target, np.float32), np.asarray(normals, np.float32)
    else:
        verts, faces = np.asarray(target[0], np.float32), np.asarray(target[1])

    def evaluate(p):
        if normals is not None:
            d, i = E.nn_brute(p.astype(np.float32), tgt, max_corr)
            s = system_from_rows(*cloud_rows(p, i, d, tgt, nrm), kernel)
        else:
            face, d2, closest, _ = P.closest_brute(p.astype(np.float32), verts, faces)
            face = np.where(d2 <= float(max_corr) * float(max_corr), face, -1)
            s = system_from_rows(*surface_rows(p, face, d2, closest, verts, faces), kernel)
        k = s["k_corr"]
        return s, (k / len(p) if k else 0.0), (math.sqrt(float(s["sums"][29]) / k) if k else 0.0)

    s, fit, rmse = evaluate(cur)
    iterations, degenerate = 0, False
    for it in range(max_iter):
        x = ldlt_solve(s["A"], s["b"])
        if x is None:
            degenerate = True
            break
        upd = update_matrix(x)
        T = matmul4(upd, T)
        cur = E.transform(cur, upd)
        prev = (fit, rmse)
        s, fit, rmse = evaluate(cur)
        iterations = it + 1
        if abs(prev[0] - fit) < rel_fitness and abs(prev[1] - rmse) < rel_rmse:
            break
    used = s["k_used"]
    return dict(transformation=T, fitness=fit, inlier_rmse=rmse, iterations=iterations, used=used, degenerate=degenerate,
                residual_rmse=math.sqrt(float(s["sums"][27]) / used) if used else 0.0)


# ---- shared inputs --------------------------------------------------------------------------------------------------------------

MOTION = ([0.2, 1.0, -0.4], 3.0, [0.03, -0.02, 0.025])
K_EXACT = 2.0 ** -6                                     # the kernel width of the synthetic rows: some have |r| == K_EXACT exactly


def box_case(outliers=0):
    """dict of the box case: the mesh, 4000 target samples (seed 1) with their face normals, 1500 source samples (seed 2; ``outliers``
    uniform points of the box scaled by 1.05 appended, default_rng(3)) moved by MOTION and rounded to fp32, and the 4x4 that undoes it"""
    v, f = P.box_mesh()
    tgt, tface = E.sample_surface(v, f, 4000, 1)
    src, _ = E.sample_surface(v, f, 1500, 2)
    if outliers:
        lo, hi = 1.05 * v.min(0).astype(np.float64), 1.05 * v.max(0).astype(np.float64)
        src = np.concatenate([src, (lo + np.random.default_rng(3).random((outliers, 3)) * (hi - lo)).astype(np.float32)])
    M = E.rigid(*MOTION)
    moved = E.transform(src.astype(np.float64), M).astype(np.float32)
    return dict(verts=v, faces=f, target=tgt, normals=face_unit_normals(v, f)[tface].astype(np.float32), source=moved,
                truth=np.linalg.inv(M))


def _unit(rng, n):
    x = rng.normal(size=(n, 3))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _exact_rows(p, q_z, rows, normal_z=1.0):
    """make |r| == K_EXACT exactly in ``rows`` whose normal is (0, 0, +-1): p_z = q_z +- K_EXACT, both exact in float64"""
    sign = np.where(np.arange(len(rows)) % 2 == 0, 1.0, -1.0)
    p[rows, 2] = q_z[rows] + sign * K_EXACT


def synthetic_cloud(n, seed=0, drop="third", scale=1.0, offset=0.02):
    """arguments of plane_system in cloud mode for n rows: 1000 targets with random unit normals, of which target 0 has the normal
    (0, 0, 1), target 1 a zero and target 2 a NaN one; rows 5, 11, ... have |r| == K_EXACT exactly; ``drop``: "third" leaves every
    third row without a correspondence, "all" every row, None none"""
    rng = np.random.default_rng(seed)
    m = 1000
    targets = (np.round(rng.uniform(-1, 1, (m, 3)) * 1024) / 1024 * scale).astype(np.float32)
    normals = _unit(rng, m)
    normals[0] = (0, 0, 1)
    normals[1] = 0
    normals[2] = (np.nan, 0.5, 0.5)
    idx = rng.integers(0, m, n).astype(np.int32)
    idx[7::13] = rng.integers(0, 3, len(idx[7::13]))
    exact = np.arange(5, n, 6)
    idx[exact] = 0
    q = targets[idx].astype(np.float64)
    cur = q + rng.normal(0, offset, (n, 3))
    _exact_rows(cur, q[:, 2], exact)
    dist = np.sqrt(((cur - q) ** 2).sum(1)).astype(np.float32)
    if drop == "third":
        idx[::3] = -1
    elif drop == "all":
        idx[:] = -1
    return dict(cur=cur, idx=idx, dist=dist, targets=targets, normals=normals)


def synthetic_surface(n, seed=0, drop="third"):
    """arguments of plane_system in surface mode for n rows: 300 vertices and 500 random faces, of which face 0 lies in z = 0 (normal
    (0, 0, 1) exactly) and face 1 has no area; rows 5, 11, ... have |r| == K_EXACT exactly"""
    rng = np.random.default_rng(seed + 100)
    verts = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    verts[:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    faces = np.stack([rng.permutation(300)[:3] for _ in range(500)]).astype(np.int32)
    faces[0] = (0, 1, 2)
    faces[1] = (3, 3, 4)
    face = rng.integers(0, 500, n).astype(np.int32)
    face[7::13] = rng.integers(0, 2, len(face[7::13]))
    exact = np.arange(5, n, 6)
    face[exact] = 0
    closest = (np.round(rng.uniform(-1, 1, (n, 3)) * 1024) / 1024).astype(np.float32)
    cur = closest.astype(np.float64) + rng.normal(0, 0.02, (n, 3))
    _exact_rows(cur, closest[:, 2].astype(np.float64), exact)
    d2 = ((cur - closest) ** 2).sum(1)
    if drop == "third":
        face[::3] = -1
    elif drop == "all":
        face[:] = -1
    return dict(cur=cur, face_idx=face, d2=d2, closest=closest, verts=verts, faces=faces)


def large_coordinate_cloud(n, seed=5):
    """cloud-mode rows with coordinates near 1e3 and residuals near 1e-6: every source point lies 1e-6 off its target's plane and 0.05
    along it, so the three products of r are inexact in float64 and cancel to four digits, and the products of a = p x n to nine: the
    bits of the sums follow the order of the additions and the rounding of every product"""
    rng = np.random.default_rng(seed)
    m = 1000
    targets = rng.uniform(500, 1500, (m, 3)).astype(np.float32)
    normals = _unit(rng, m)
    idx = rng.integers(0, m, n).astype(np.int32)
    nn = normals[idx].astype(np.float64)
    along = rng.normal(0, 0.05, (n, 3))
    along = along - (along * nn).sum(1, keepdims=True) / (nn * nn).sum(1, keepdims=True) * nn
    cur = targets[idx].astype(np.float64) + along + rng.normal(0, 1e-6, (n, 1)) * nn
    dist = np.sqrt(((cur - targets[idx]) ** 2).sum(1)).astype(np.float32)
    return dict(cur=cur, idx=idx, dist=dist, targets=targets, normals=normals)
