"""numpy float64 oracle of the closest point on a triangle mesh (include/nicer_slam_amd.h Section 14, csrc/mesh_closest.hip): a brute
force over all faces in the header's operation order -- numpy rounds every elementwise operation on its own, which is the contract --
and the surface="mesh" metric arithmetic of nicer_slam_amd/mesh_eval.py, plus the meshes the tests share."""
import numpy as np

F_THRESHOLDS = (0.010, 0.015, 0.020)
COMPLETION_RATIO_THRESHOLD = 0.05


def face_causes(verts, faces):
    """[F] int: 0 = usable, else the FIRST cause the face is skipped for: 1 an index outside [0, V), 2 a non-finite vertex,
    3 ab x ac exactly (0, 0, 0) in float64."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)
    V = v.shape[0]
    cause = np.zeros(f.shape[0], np.int64)
    bad_idx = ((f < 0) | (f >= V)).any(1)
    cause[bad_idx] = 1
    fc = np.where(bad_idx[:, None], 0, f)
    a, b, c = v[fc[:, 0]], v[fc[:, 1]], v[fc[:, 2]]
    nonfinite = ~(np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1))
    cause[(cause == 0) & nonfinite] = 2
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    cause[(cause == 0) & (nx == 0) & (ny == 0) & (nz == 0)] = 3
    return cause


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def pair_closest(q, a, b, c):
    """(p [..., 3], d2 [...]) of float64 q against faces (a, b, c), broadcast; the header's lines 1-7"""
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = q - a, q - b, q - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        e = 1.0 / ((va + vb) + vc)
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        s = np.select(tests, [zero, one, d1 / (d1 - d3), zero, zero, 1.0 - w], vb * e)
        t = np.select(tests, [zero, zero, zero, one, d2 / (d2 - d6), w], vc * e)
        p = (a + s[..., None] * ab) + t[..., None] * ac
        r = q - p
        return p, (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]


def closest_brute(queries, verts, faces, pairs=400_000):
    """(face [M] int64, d2 [M] float64, closest [M, 3] fp32, totals [3]) by brute force: the smallest d2 over the usable faces (NaN
    never wins), ties to the lowest index; a non-finite query (-1, NaN), no usable face (-1, +inf); closest NaN in both cases."""
    q = np.asarray(queries, np.float32).astype(np.float64).reshape(-1, 3)
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    cause = face_causes(verts, f)
    totals = np.array([(cause == k).sum() for k in (1, 2, 3)], np.int64)
    use = np.nonzero(cause == 0)[0]
    M = q.shape[0]
    face = np.full(M, -1, np.int64)
    best = np.full(M, np.inf)
    close = np.full((M, 3), np.nan)
    if use.size:
        a, b, c = v[f[use, 0]][None], v[f[use, 1]][None], v[f[use, 2]][None]
        step = max(1, pairs // use.size)
        for lo in range(0, M, step):
            p, d2 = pair_closest(q[lo:lo + step, None, :], a, b, c)
            d2 = np.where(np.isnan(d2), np.inf, d2)
            k = d2.argmin(1)                         # the first minimum = the lowest face index (use is ascending)
            rows = np.arange(k.size)
            found = d2[rows, k] < np.inf
            best[lo:lo + step] = d2[rows, k]
            face[lo:lo + step] = np.where(found, use[k], -1)
            close[lo:lo + step] = np.where(found[:, None], p[rows, k], np.nan)
    bad = ~np.isfinite(q).all(1)
    face[bad] = -1
    best[bad] = np.nan
    close[bad] = np.nan
    with np.errstate(over="ignore"):
        return face, best, close.astype(np.float32), totals


def face_normals(verts, faces):
    """unit normals [F, 3] float64 of usable faces, in the operation order of mesh_eval._face_normals"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-300)


def surface_metrics(d_acc, d_com, dot_acc, dot_com):
    """the surface="mesh" arithmetic: d_acc distances of the reconstruction's samples to the ground-truth mesh, d_com of the
    ground truth's samples to the reconstruction's mesh; dot_* = n_sample . n_closest_face for the same pairs"""
    acc, com = np.asarray(d_acc, np.float64), np.asarray(d_com, np.float64)
    out = {"accuracy": acc.mean(), "completion": com.mean(),
           "completion ratio": (com < COMPLETION_RATIO_THRESHOLD).astype(np.float64).mean(),
           "normals": 0.5 * np.abs(dot_com).mean() + 0.5 * np.abs(dot_acc).mean(),
           "chamfer-L1": 0.5 * (com.mean() + acc.mean()),
           "chamfer-L2": 0.5 * ((com * com).mean() + (acc * acc).mean())}
    for key, th in zip(("f-score", "f-score-15", "f-score-20"), F_THRESHOLDS):
        p, r = (acc <= th).astype(np.float64).mean(), (com <= th).astype(np.float64).mean()
        out[key] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return {k: float(x) for k, x in out.items()}


# ---- shared meshes ----------------------------------------------------------------------------------------------------------------

def box_mesh(lo=(-1.0, -0.5, -0.25), hi=(1.0, 0.5, 0.25)):
    """the 12 triangles of an axis-aligned box (outward winding)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def box_distance(q, lo=(-1.0, -0.5, -0.25), hi=(1.0, 0.5, 0.25)):
    """closed form of the distance from q [M, 3] float64 to the SURFACE of the box"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = np.maximum(np.maximum(lo - q, q - hi), 0.0)
    outside = np.sqrt((out * out).sum(1))
    inside = np.minimum(q - lo, hi - q).min(1)
    return np.where((out > 0).any(1), outside, inside)


def latlong_sphere(n_lat=24, n_lon=48, r=1.0):
    """(verts [(n_lat + 1) (n_lon + 1), 3] fp32, faces [2 n_lat n_lon, 3] int32, n_degenerate): quads of a latitude-longitude grid
    split in two.  The seam column is duplicated and each pole is a row of coincident vertices, so in each pole row one triangle
    of every quad has two coincident corners: 2 n_lon zero-area faces by construction."""
    th = np.linspace(0.0, np.pi, n_lat + 1)
    ph = np.linspace(0.0, 2 * np.pi, n_lon + 1)
    T, P = np.meshgrid(th, ph, indexing="ij")
    sin_t = np.sin(T)
    sin_t[0] = 0.0
    sin_t[-1] = 0.0                                  # the poles exactly: every vertex of a pole row is the same point
    v = np.stack([r * sin_t * np.cos(P), r * sin_t * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange((n_lat + 1) * (n_lon + 1)).reshape(n_lat + 1, n_lon + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    f = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3).astype(np.int32)
    return v, f, 2 * n_lon


def sag(verts, faces, r=1.0):
    """the largest sag of a mesh inscribed in the sphere of radius r about 0: r less the least distance of a face plane from
    the centre, over the usable faces"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)[face_causes(verts, faces) == 0]
    n = face_normals(verts, f)
    return float(r - np.abs((n * v[f[:, 0]]).sum(1)).min())
