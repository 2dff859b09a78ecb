"""numpy restatement of the mesh-evaluation path (nicer_slam_amd/mesh_eval.py, csrc/mesh_eval.hip) for the tests:
brute-force fp32 nearest neighbours with the tie and radius rules, surface sampling from the Philox stream, the arithmetic of
eval_rec.py's eval_pointcloud / calc_3d_metric, and open3d's point-to-point ICP loop."""
import math

import numpy as np

F_THRESHOLDS = (0.010, 0.015, 0.020)


# ---- nearest neighbours -----------------------------------------------------------------------------------------------------

def nn_brute(queries, targets, max_dist=math.inf, chunk=512):
    """(dist fp32 [m], idx int64 [m]): smallest d2 = (dx*dx + dy*dy) + dz*dz in fp32 (dk = t_k - q_k, each operation rounded),
    ties to the lowest index; non-finite targets never chosen; non-finite query -> (NaN, -1); with a radius only d2 <
    fp32(max_dist^2) counts, none -> (+inf, -1)."""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    t = np.asarray(targets, np.float32).reshape(-1, 3)
    valid = np.isfinite(t).all(1)
    strict = max_dist < math.inf
    r2 = np.float32(max_dist * max_dist) if strict else np.float32(np.inf)
    dist = np.full(len(q), np.inf, np.float32)
    idx = np.full(len(q), -1, np.int64)
    ar = np.arange(len(t))
    with np.errstate(over="ignore", invalid="ignore"):
        for lo in range(0, len(q), chunk):
            qq = q[lo:lo + chunk]
            dx, dy, dz = (t[None, :, k] - qq[:, None, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(valid[None, :], d2, np.float32(np.nan))
            ok = (d2 < r2) if strict else valid[None, :] & ~np.isnan(d2)
            best = np.where(ok, d2, np.float32(np.inf)).min(1)
            hit = ok & (d2 == best[:, None])
            first = np.where(hit, ar[None, :], len(t)).min(1)
            found = first < len(t)
            idx[lo:lo + chunk] = np.where(found, first, -1)
            dist[lo:lo + chunk] = np.where(found, np.sqrt(best), np.float32(np.inf))
    bad = ~np.isfinite(q).all(1)
    idx[bad] = -1
    dist[bad] = np.nan
    return dist, idx


# ---- Philox4x32-10 and surface sampling -------------------------------------------------------------------------------------

_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Vectorised Philox4x32-10: ctr uint32 [n, 4], key (k0, k1) -> uint32 [n, 4]."""
    c = [np.asarray(ctr, np.uint64)[:, i] for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def face_areas(verts, faces):
    """0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = (v1 - v0) x (v2 - v0), float64 from the fp32 vertices."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def area_cumsum(areas, block=1024):
    """cum[f] = boff[b] + local[f]: sequential inclusive scan within blocks of 1024 faces, sequential sum of the block totals."""
    F = len(areas)
    nb = (F + block - 1) // block
    s = np.zeros(nb * block)
    s[:F] = areas
    s = np.cumsum(s.reshape(nb, block), axis=1)           # (numpy's cumsum adds in order)
    boff = np.zeros(nb + 1)
    c = 0.0
    for b in range(nb):
        boff[b] = c
        c = c + s[b, -1]
    boff[nb] = c
    cum = (boff[:nb, None] + s).reshape(-1)[:F]
    return cum, c


def sample_surface(verts, faces, n, seed):
    """(points fp32 [n, 3], face_idx [n]) as nsa_surface_sample."""
    v = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64)
    cum, total = area_cumsum(face_areas(v, f))
    s = np.arange(n, dtype=np.uint64)
    ctr = np.stack([s, 0 * s, 0 * s, 0 * s], 1)
    c = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    x = ((c[:, 0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24 * total
    face = np.searchsorted(cum, x, side="left")
    a = (c[:, 1] >> 8).astype(np.float32) * np.float32(2.0 ** -24)
    b = (c[:, 2] >> 8).astype(np.float32) * np.float32(2.0 ** -24)
    flip = (a + b) > np.float32(1.0)
    a = np.where(flip, np.float32(1.0) - a, a)
    b = np.where(flip, np.float32(1.0) - b, b)
    v0, v1, v2 = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    p = (v0 + a[:, None] * (v1 - v0)) + b[:, None] * (v2 - v0)
    return p.astype(np.float32), face


def face_normals(verts, faces):
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-300)


# ---- metrics ------------------------------------------------------------------------------------------------------------------

def metrics(acc_dist, acc_idx, com_dist, com_idx, rec_normals, gt_normals):
    """eval_pointcloud + completion_ratio arithmetic from the two nearest-neighbour results (accuracy: rec -> gt, completion:
    gt -> rec) and the samples' unit normals."""
    acc, com = np.asarray(acc_dist, np.float64), np.asarray(com_dist, np.float64)
    n_acc = np.abs((gt_normals[acc_idx] * rec_normals).sum(-1)).mean()
    n_com = np.abs((rec_normals[com_idx] * gt_normals).sum(-1)).mean()
    out = {"accuracy": acc.mean(), "completion": com.mean(), "completion ratio": (com < 0.05).mean(),
           "normals": 0.5 * n_com + 0.5 * n_acc, "chamfer-L1": 0.5 * (com.mean() + acc.mean()),
           "chamfer-L2": 0.5 * ((com ** 2).mean() + (acc ** 2).mean())}
    for key, th in zip(("f-score", "f-score-15", "f-score-20"), F_THRESHOLDS):
        p, r = (acc <= th).mean(), (com <= th).mean()
        out[key] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return out


# ---- ICP ----------------------------------------------------------------------------------------------------------------------

def transform(p, T):
    R, t = T[:3, :3], T[:3, 3]
    return np.stack([((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k] for k in range(3)], -1)


def kabsch(src, tgt):
    """Umeyama without scale: R = U diag(1, 1, sign det(U) det(V)) V^T of the cross-covariance, t = mt - R ms."""
    ms, mt = src.mean(0), tgt.mean(0)
    cov = (tgt - mt).T @ (src - ms) / len(src)
    U, _, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ S @ Vt
    T[:3, 3] = mt - T[:3, :3] @ ms
    return T


def icp(source, target, max_corr=0.1, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, nn=None):
    """open3d registration_icp, point to point, ICPConvergenceCriteria(rel_fitness, rel_rmse, max_iter)."""
    nn = nn or nn_brute
    src = np.asarray(source, np.float32).astype(np.float64)
    tgt = np.asarray(target, np.float32)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    cur = transform(src, T)

    def evaluate(p):
        d, i = nn(p.astype(np.float32), tgt, max_corr)
        ok = i >= 0
        k = int(ok.sum())
        if k == 0:
            return 0.0, 0.0, ok, i
        d64 = d[ok].astype(np.float64)
        return k / len(p), math.sqrt((d64 * d64).sum() / k), ok, i

    fit, rmse, ok, i = evaluate(cur)
    it = 0
    for it in range(max_iter):
        upd = kabsch(cur[ok], tgt[i[ok]].astype(np.float64)) if ok.any() else np.eye(4)
        T = upd @ T
        cur = transform(cur, upd)
        prev = (fit, rmse)
        fit, rmse, ok, i = evaluate(cur)
        if abs(prev[0] - fit) < rel_fitness and abs(prev[1] - rmse) < rel_rmse:
            break
    return dict(transformation=T, fitness=fit, inlier_rmse=rmse, iterations=it + 1 if max_iter > 0 else 0)


def rigid(axis, angle_deg, t):
    """4x4 rotation about ``axis`` by ``angle_deg`` followed by translation ``t`` (Rodrigues)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    T[:3, 3] = t
    return T
