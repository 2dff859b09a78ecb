"""numpy restatement of header Section 23 (csrc/mesh_fill.hip, nicer_slam_amd/mesh_fill.py) for the tests: the successor
of every boundary half-edge by rotation inside the face fan, pinch marks, loops as cycles of the successor with the smallest
half-edge id leading, the per-loop table in rank order, and the polar patch.  Float64, + - * / only, every sum in rank order starting
from zero.  Needs numpy and tests/topology_ref.py only."""
import numpy as np

import topology_ref as T

CLASSES = ("filled", "nonfinite", "pinched", "too_many_edges", "too_large", "folded")
FILLED, NONFINITE, PINCHED, TOO_MANY, TOO_LARGE, FOLDED = range(6)
TOTALS = ("n_boundary", "n_loops", "n_filled", "n_nonfinite", "n_pinched", "n_too_many_edges", "n_too_large", "n_folded",
          "n_open_chain", "n_new_verts", "n_new_faces", "status")
INT_COLS = ("leader", "n", "start", "class", "rings", "new_verts", "new_faces", "vert_offset", "face_offset")
REAL_COLS = 18                 # centre 3, mean colour 3, box lo 3, box hi 3, D2, R2, L2, A 3


def n_rounds(B):
    """ceil(log2(max(B, 2))) + 1"""
    return int(max(B, 2) - 1).bit_length() + 1


def trace(faces, n_verts, names=None):
    """the integer part: dict with ``halfedges`` [B] (ascending), ``next`` [B] (item indices), ``blocked``, ``pinch``, ``leader``
    (item index, -1 on an open chain), ``rank``, ``loop`` (-1 on an open chain), ``loop_leader`` / ``loop_n`` / ``loop_start`` [L],
    ``order`` [sum n] (half-edge ids) and ``status``.  ``names``: the face list the topology is read from (welded names); the start
    vertices of the pinch test are read from it as well."""
    f = np.asarray(faces if names is None else names, np.int64).reshape(-1, 3)
    F, V = len(f), int(n_verts)
    t = T.edge_table(f, V)
    fe = t["face_edges"].reshape(-1)
    count, fwd, start, he = t["edge_count"], t["edge_forward"], t["edge_start"], t["edge_halfedges"]
    is_b = np.zeros(3 * F, bool)
    is_b[fe >= 0] = count[fe[fe >= 0]] == 1
    bh = np.nonzero(is_b)[0]
    B = len(bh)
    slot = np.full(3 * F, -1, np.int64)
    slot[bh] = np.arange(B)
    nxt, blocked, status = np.arange(B), np.zeros(B, bool), 0
    for i, h in enumerate(bh):
        g = 3 * (h // 3) + (h % 3 + 1) % 3
        steps = 0
        while not is_b[g]:
            e = fe[g]
            if count[e] != 2 or fwd[e] != 1:
                blocked[i] = True
                break
            if steps >= F:
                blocked[i], status = True, status | 1
                break
            steps += 1
            a, b = he[start[e]], he[start[e] + 1]
            tw = b if a == g else a
            g = 3 * (tw // 3) + (tw % 3 + 1) % 3
        if not blocked[i]:
            nxt[i] = slot[g]
    sv = f.reshape(-1)[bh] if B else np.zeros(0, np.int64)
    pinch = np.bincount(sv, minlength=max(V, 1))[sv] >= 2 if B else np.zeros(0, bool)
    # open chains by pointer jumping (the device's rounds); leaders and ranks by walking every cycle
    p, term = nxt.copy(), blocked.copy()
    for _ in range(n_rounds(B)):
        term = term | term[p]
        p = p[p]
    leader, rank, loop = np.full(B, -1, np.int64), np.zeros(B, np.int64), np.full(B, -1, np.int64)
    heads, lens, order = [], [], []
    for i in range(B):
        if term[i] or leader[i] >= 0:
            continue
        j, k = i, 0
        while True:
            leader[j], rank[j], loop[j] = i, k, len(heads)
            order.append(bh[j])
            j, k = nxt[j], k + 1
            if j == i:
                break
        heads.append(bh[i])
        lens.append(k)
    lens = np.array(lens, np.int64)
    return dict(halfedges=bh, next=nxt, blocked=blocked, pinch=pinch, open_chain=term, leader=leader, rank=rank, loop=loop,
                loop_leader=np.array(heads, np.int64), loop_n=lens,
                loop_start=np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64) if len(lens) else np.zeros(0, np.int64),
                order=np.array(order, np.int64), status=status)


def _seq_sum(x):
    """the sum of the rows of x in order, starting from zero"""
    return np.cumsum(np.concatenate([np.zeros((1,) + x.shape[1:]), x]), axis=0)[-1]


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def _first_extreme(X, ext):
    """per column the first row of X equal to ext (the value a running ``if p < lo: lo = p`` keeps: -0 and +0 compare equal)"""
    return X[np.argmax(X == ext[None], axis=0), np.arange(X.shape[1])]


def loop_table(verts, faces, tr, colors=None, max_edges=None, max_size=None, rings="auto", max_rings=64, skip_folded=True):
    """(ints int64 [L, 9] in INT_COLS order, reals float64 [L, 18], totals dict)"""
    v32 = np.ascontiguousarray(verts, np.float32)
    X = v32.astype(np.float64)
    C = None if colors is None else np.ascontiguousarray(colors, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1)
    L = len(tr["loop_n"])
    ints, reals = np.zeros((L, len(INT_COLS)), np.int64), np.zeros((L, REAL_COLS))
    slot = {int(h): i for i, h in enumerate(tr["halfedges"])}
    vo = fo = 0
    with np.errstate(all="ignore"):
        for l in range(L):
            n, s = int(tr["loop_n"][l]), int(tr["loop_start"][l])
            hs = tr["order"][s:s + n]
            P = X[f[hs]]
            nd = np.float64(n)
            cls, K = None, 0
            if not np.isfinite(P).all():
                cls = NONFINITE
            else:
                c = _seq_sum(P) / nd
                cm = _seq_sum(C[f[hs]]) / nd if C is not None else np.zeros(3)
                lo, hi = _first_extreme(P, P.min(0)), _first_extreme(P, P.max(0))
                e = hi - lo
                D2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                d = P - c[None]
                R2 = _seq_sum(_dot(d, d)) / nd
                Pn = np.roll(P, -1, axis=0)
                g = Pn - P
                L2 = _seq_sum(_dot(g, g)) / nd
                ni = _cross(Pn - c[None], d)
                A = _seq_sum(ni)
                reals[l] = np.concatenate([c, cm, lo, hi, [D2, R2, L2], A])
                if isinstance(rings, str):
                    K = 1
                    while K < max_rings and not (np.float64(K) * np.float64(K)) * L2 >= R2:
                        K += 1
                else:
                    K = int(rings)
                if any(tr["pinch"][slot[int(h)]] for h in hs):
                    cls = PINCHED
                elif max_edges is not None and n > max_edges:
                    cls = TOO_MANY
                elif max_size is not None and D2 > np.float64(max_size) * np.float64(max_size):
                    cls = TOO_LARGE
                elif skip_folded and (_dot(ni, A[None]) <= 0.0).any():
                    cls = FOLDED
                else:
                    cls = FILLED
            nv, nf = ((K - 1) * n + 1, n * (2 * K - 1)) if cls == FILLED else (0, 0)
            ints[l] = (tr["loop_leader"][l], n, s, cls, K, nv, nf, vo, fo)
            vo, fo = vo + nv, fo + nf
    totals = dict(n_boundary=len(tr["halfedges"]), n_loops=L, n_open_chain=int(tr["open_chain"].sum()), n_new_verts=vo, n_new_faces=fo,
                  status=tr["status"])
    for k, name in enumerate(CLASSES):
        totals["n_" + name] = int((ints[:, 3] == k).sum())
    return ints, reals, {k: int(totals[k]) for k in TOTALS}


def emit(verts, faces, tr, ints, reals, colors=None):
    """(new verts float32 [n_new_verts, 3], new colours or None, new faces int64 [n_new_faces, 3])"""
    v32 = np.ascontiguousarray(verts, np.float32)
    X = v32.astype(np.float64)
    V = len(X)
    C = None if colors is None else np.ascontiguousarray(colors, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1)
    nv, nf, nc = [np.zeros((0, 3), np.float32)], [np.zeros((0, 3), np.int64)], [np.zeros((0, 3), np.float32)]
    for l in range(len(ints)):
        _, n, s, cls, K, _, _, vo, _ = (int(x) for x in ints[l])
        if cls != FILLED:
            continue
        r0 = f[tr["order"][s:s + n]]
        c, cm = reals[l, 0:3], reals[l, 3:6]
        ring = lambda j: r0 if j == 0 else V + vo + (j - 1) * n + np.arange(n)
        centre = V + vo + (K - 1) * n
        for j in range(1, K):
            tj = np.float64(K - j) / np.float64(K)
            nv.append((c[None] + tj * (X[r0] - c[None])).astype(np.float32))
            if C is not None:
                nc.append((cm[None] + tj * (C[r0] - cm[None])).astype(np.float32))
        nv.append(c[None].astype(np.float32))
        if C is not None:
            nc.append(cm[None].astype(np.float32))
        for j in range(K - 1):
            a, b = ring(j), ring(j + 1)
            an, bn = np.roll(a, -1), np.roll(b, -1)
            nf.append(np.stack([np.stack([an, a, b], 1), np.stack([an, b, bn], 1)], 1).reshape(-1, 3))
        a = ring(K - 1)
        nf.append(np.stack([np.roll(a, -1), a, np.full(n, centre)], 1))
    return np.concatenate(nv), None if C is None else np.concatenate(nc), np.concatenate(nf)


def boundary_loops(faces, n_verts):
    """(loop_start [L + 1], vertices in rank order, trace)"""
    tr = trace(faces, n_verts)
    f = np.asarray(faces, np.int64).reshape(-1)
    return np.concatenate([tr["loop_start"], [len(tr["order"])]]).astype(np.int64), f[tr["order"]], tr


def fill_holes(mesh, max_edges=None, max_size=None, rings="auto", max_rings=64, skip_folded=True, names=None):
    """the statement of ``mesh_fill.fill_holes`` without fairing and normals: a dict with ``verts`` float32, ``faces`` int32,
    ``colors`` when given, and the report parts ``trace``, ``ints``, ``reals``, ``totals``, ``new_vertex``"""
    v32 = np.ascontiguousarray(mesh["verts"], np.float32).reshape(-1, 3)
    f = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    col = mesh.get("colors")
    tr = trace(f, len(v32), names)
    ints, reals, totals = loop_table(v32, f, tr, col, max_edges, max_size, rings, max_rings, skip_folded)
    nv, nc, nf = emit(v32, f, tr, ints, reals, col)
    out = dict(verts=np.concatenate([v32, nv]), faces=np.concatenate([f, nf]).astype(np.int32), trace=tr, ints=ints, reals=reals,
               totals=totals, new_vertex=np.concatenate([np.zeros(len(v32), bool), np.ones(len(nv), bool)]))
    if col is not None:
        out["colors"] = np.concatenate([np.ascontiguousarray(col, np.float32).reshape(-1, 3), nc])
    return out


# ---- meshes whose answers can be derived by hand ------------------------------------------------------------------------------------

def grid_without(n, cells):
    """smooth_ref.grid_mesh(n) without the listed cells (i, j)"""
    import smooth_ref
    v, f = smooth_ref.grid_mesh(n)
    m = n - 1
    ci, cj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    gone = np.zeros((m, m), bool)
    for i, j in cells:
        gone[i, j] = True
    keep = ~gone[ci.reshape(-1), cj.reshape(-1)]
    return v, f[np.concatenate([keep, keep])]


def open_cylinder(n=12, m=4, height=4.0):
    """n x m quads around the z axis, unit radius, outward, open at both ends"""
    ang = 2.0 * np.pi * np.arange(n) / n
    z = height * np.arange(m + 1) / m
    v = np.stack([np.tile(np.cos(ang), m + 1), np.tile(np.sin(ang), m + 1), np.repeat(z, n)], 1).astype(np.float32)
    f = []
    for k in range(m):
        for i in range(n):
            a, b = k * n + i, k * n + (i + 1) % n
            c, d = a + n, b + n
            f += [[a, b, d], [a, d, c]]
    return v, np.array(f, np.int32)



def with_colors(mesh, seed=3):
    v = np.asarray(mesh["verts"])
    return dict(mesh, colors=np.random.default_rng(seed).uniform(0.0, 1.0, (len(v), 3)).astype(np.float32))


def table_cases():
    """{name: (mesh, keywords)}: the rows of DESIGN 4v, some of them with colours"""
    import simplify_ref
    import smooth_ref
    mesh = lambda v, f: dict(verts=np.ascontiguousarray(v, np.float32), faces=np.ascontiguousarray(f, np.int32))
    named = lambda fV: mesh(smooth_ref.index_only_mesh(*fV), fV[0])
    m = T.mc_mesh("sphere", 16, (0.7, 0.0, 0.0))
    cut = mesh(m["verts"], m["faces"])
    grid9 = mesh(*smooth_ref.grid_mesh(9, hole=(2, 3, 3)))
    return {
        "cut sphere, one ring": (cut, dict(rings=1)),
        "cut sphere": (with_colors(cut), {}),
        "grid with a hole, small loops only": (grid9, dict(max_edges=12)),
        "grid with a hole": (with_colors(grid9), {}),
        "grid without two cells": (mesh(*grid_without(7, [(1, 1), (4, 4)])), dict(rings=1)),
        "grid without two touching cells": (mesh(*grid_without(7, [(2, 2), (3, 3)])), dict(rings=1)),
        "grid without two touching cells, other diagonal": (mesh(*grid_without(7, [(2, 3), (3, 2)])), dict(rings=1)),
        "open tetrahedron": (mesh(simplify_ref.TET_V, simplify_ref.TET_F[:3]), {}),
        "open cylinder": (with_colors(mesh(*open_cylinder())), {}),
        "moebius strip": (named(T.moebius(8)), {}),
        "fan": (named(T.fan(300)), {}),
        "strip": (named(T.strip(50)), {}),
        "strip, folded kept": (with_colors(named(T.strip(50))), dict(skip_folded=False)),
        "cut sphere, three rings": (cut, dict(rings=3)),
        "grid with a hole, size limit": (grid9, dict(max_size=5.0)),
    }
