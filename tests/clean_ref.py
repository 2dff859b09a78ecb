"""numpy restatement of the mesh clean-up path (nicer_slam_amd/mesh_clean.py, csrc/mesh_clean.hip, the scaled ICP of
mesh_eval.py) for the tests: connected components by shared vertex index with a plain union-find (smaller root wins),
the per-component table, the three selections, the order-preserving compaction, the similarity transform, Umeyama and the ICP
loop of eval_ref.icp with a ``with_scaling`` switch.  Needs numpy only."""
import math

import numpy as np

import eval_ref as E


def valid_faces(faces, n_verts):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < n_verts)).all(1)


def components(faces, n_verts):
    """(vertex_label [V], face_label [F], n_components, n_referenced); label = the smallest vertex index of the component,
    -1 for a vertex no valid face uses / an invalid face."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = int(n_verts)
    ok = valid_faces(f, V)
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    used = np.zeros(V, bool)
    for a, b, c in f[ok].tolist():
        used[a] = used[b] = used[c] = True
        unite(a, b)
        unite(b, c)
    vl = np.full(V, -1, np.int64)
    for v in np.nonzero(used)[0].tolist():
        vl[v] = find(v)
    fl = np.full(len(f), -1, np.int64)
    fl[ok] = vl[f[ok, 0]]
    return vl, fl, int((vl == np.arange(V)).sum()), int(used.sum())


def _ord(x):
    """order-preserving integer image of fp32 values (-0 below +0)"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def _unord(e):
    e = np.asarray(e, np.int64)
    u = np.where(e & 0x80000000, e ^ 0x80000000, 0xFFFFFFFF - e).astype(np.uint32)
    return u.view(np.float32)


def component_stats(verts, faces):
    """dict(label, n_faces, n_verts, area (math.fsum of eval_ref.face_areas), lo, hi, vertex_comp, face_comp, n_components);
    components in ascending label order."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    vl, fl, C, _ = components(f, V)
    label = np.nonzero(vl == np.arange(V))[0]
    rank = np.full(V + 1, -1, np.int64)
    rank[label] = np.arange(C)
    vc, fc = rank[vl], rank[fl]                      # (-1 indexes the spare last slot, which holds -1)
    ok = fc >= 0
    area_f = np.zeros(len(f))
    fin = np.isfinite(v).all(1)
    good = ok.copy()
    good[ok] = fin[f[ok]].all(1)
    area_f[good] = E.face_areas(v, f[good])
    area = _fsum_by(area_f, fc, C)
    lo = np.full((C, 3), 0xFFFFFFFF, np.int64)
    hi = np.zeros((C, 3), np.int64)
    lo[:] = _ord(np.float32(np.inf))
    hi[:] = _ord(np.float32(-np.inf))
    e = _ord(v)
    for k in range(3):
        m = (vc >= 0) & np.isfinite(v[:, k])
        np.minimum.at(lo[:, k], vc[m], e[m, k])
        np.maximum.at(hi[:, k], vc[m], e[m, k])
    return dict(label=label, n_faces=np.bincount(fc[ok], minlength=C), n_verts=np.bincount(vc[vc >= 0], minlength=C), area=area,
                lo=_unord(lo), hi=_unord(hi), vertex_comp=vc, face_comp=fc, n_components=C)


def _fsum_by(values, comp, C):
    order = np.argsort(comp, kind="stable")
    comp_s, val_s = comp[order], values[order]
    start = np.searchsorted(comp_s, np.arange(C), "left")
    end = np.searchsorted(comp_s, np.arange(C), "right")
    return np.array([math.fsum(val_s[s:e].tolist()) for s, e in zip(start, end)])


def select_components(stats, verts, keep="largest", region=None):
    """bool [C]: the components kept"""
    C = stats["n_components"]
    if keep == "largest":
        kept = np.zeros(C, bool)
        kept[int(np.argmax(stats["area"]))] = True            # (argmax returns the first maximum: the smallest label)
        return kept
    lo, hi = (np.asarray(x, np.float64) for x in region)
    v = np.asarray(verts, np.float32).astype(np.float64)
    inside = ((v >= lo) & (v <= hi)).all(1) & (stats["vertex_comp"] >= 0)
    hit = np.zeros(C, bool)
    hit[stats["vertex_comp"][inside]] = True
    return hit if keep == "touching" else ~hit


def select_faces(mesh, face_mask):
    """used -> cumsum -> remap: the kept faces and the vertices they use, both in their original order"""
    f = np.asarray(mesh["faces"])
    mask = np.asarray(face_mask, bool)
    kept = f[mask].astype(np.int64)
    V = len(mesh["verts"])
    used = np.zeros(V, bool)
    used[kept.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    out = dict(mesh)
    out["faces"] = remap[kept].astype(f.dtype)
    for k in ("verts", "normals", "colors"):
        if k in mesh:
            out[k] = np.asarray(mesh[k])[used]
    return out


def keep_components(mesh, keep="largest", region=None):
    st = component_stats(mesh["verts"], mesh["faces"])
    kept = select_components(st, mesh["verts"], keep, region)
    fc = st["face_comp"]
    return select_faces(mesh, (fc >= 0) & kept[np.maximum(fc, 0)]), st, kept


def transform_mesh(mesh, T):
    """vertices: float64 ((R0 x + R1 y) + R2 z) + t rounded once to fp32; normals: the linear part, normalised, zero stays zero"""
    T = np.asarray(T, np.float64)
    out = dict(mesh)
    out["verts"] = E.transform(np.asarray(mesh["verts"], np.float32).astype(np.float64), T).astype(np.float32)
    if "normals" in mesh:
        Z = np.zeros((4, 4))
        Z[:3, :3] = T[:3, :3]
        n = E.transform(np.asarray(mesh["normals"], np.float32).astype(np.float64), Z)
        length = np.linalg.norm(n, axis=-1, keepdims=True)
        out["normals"] = np.where(length > 0, n / np.maximum(length, 1e-300), 0.0).astype(np.float32)
    return out


def similarity(axis, angle_deg, t, s):
    T = E.rigid(axis, angle_deg, t)
    T[:3, :3] *= s
    return T


def umeyama(src, tgt, with_scaling=False):
    """Umeyama's least-squares similarity (c R, t) of src onto tgt; c = 1 without scaling (eval_ref.kabsch)."""
    ms, mt = src.mean(0), tgt.mean(0)
    cov = (tgt - mt).T @ (src - ms) / len(src)
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    if with_scaling:
        var = ((src - ms) ** 2).sum() / len(src)
        R = ((D[0] * S[0, 0] + D[1] * S[1, 1]) + D[2] * S[2, 2]) / var * R
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mt - R @ ms
    return T


def icp(source, target, max_corr=0.1, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, nn=None, with_scaling=False):
    """eval_ref.icp with the update switched between Kabsch and Umeyama with scale"""
    nn = nn or E.nn_brute
    src = np.asarray(source, np.float32).astype(np.float64)
    tgt = np.asarray(target, np.float32)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    cur = E.transform(src, T)

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
        upd = umeyama(cur[ok], tgt[i[ok]].astype(np.float64), with_scaling) if ok.any() else np.eye(4)
        T = upd @ T
        cur = E.transform(cur, upd)
        prev = (fit, rmse)
        fit, rmse, ok, i = evaluate(cur)
        if abs(prev[0] - fit) < rel_fitness and abs(prev[1] - rmse) < rel_rmse:
            break
    return dict(transformation=T, fitness=fit, inlier_rmse=rmse, iterations=it + 1 if max_iter > 0 else 0)


# ---- index-order cases where chain depth and contention are the point (shared by the CPU and the GPU tests) -------------------

def adversarial_cases(n=100000, seed=7):
    """{name: (faces int32 [F, 3], n_verts)}"""
    g = np.random.default_rng(seed)
    i = np.arange(n - 2, dtype=np.int64)
    strip = np.stack([i, i + 1, i + 2], 1)
    perm = g.permutation(n)
    hub = n // 2
    j = np.arange(n - 1, dtype=np.int64)
    two = np.empty((2 * len(strip), 3), np.int64)
    two[0::2], two[1::2] = strip, strip + n
    mixed = np.array([[0, 1, 2], [-1, 3, 4], [5, 12, 6], [7, 7, 8], [2, 8, 8], [5, 6, 5], [9, 10, 2 ** 31 - 1]], np.int64)
    cases = {
        "strip": (strip, n),
        "strip reversed": (strip[::-1].copy(), n),
        "strip permuted names": (perm[strip], n),
        "star": (np.stack([np.full(n - 1, hub), j, j + 1], 1), n + 1),
        "random sparse": (g.integers(0, 3 * n, (n, 3)), 3 * n),
        "random dense": (g.integers(0, n // 2, (n, 3)), n // 2),
        "soup": (np.arange(3 * (n // 2), dtype=np.int64).reshape(-1, 3), 3 * (n // 2)),
        "two strips alternating": (two, 2 * n),
        "invalid, degenerate, trailing": (mixed, 12),
        "no faces": (np.zeros((0, 3), np.int64), 5),
    }
    return {k: (f.astype(np.int32), V) for k, (f, V) in cases.items()}
