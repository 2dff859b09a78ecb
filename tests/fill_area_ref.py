"""numpy restatement of header Section 24 (csrc/mesh_fill_area.hip, nicer_slam_amd/mesh_fill.py) for the tests: the
triangle weight, the chord mask, the interval programme diagonal by diagonal with the smallest j winning a tie, the classes, the
offsets and the faces in pre-order numbering, and ``fill_holes`` with ``method="auto" | "min_area"`` on top of tests/fill_ref.py's
trace and loop table.  Float64, + - * rounded one by one, one square root per triangle.  Also a brute-force enumeration of all
triangulations for small loops and the meshes of the tests.  Needs numpy, tests/fill_ref.py and tests/topology_ref.py only."""
import numpy as np

import fill_ref as R
import topology_ref as T

AREA_CLASSES = ("area_filled", "area_too_many_edges", "no_triangulation")
NOT_SELECTED, AREA_FILLED, AREA_TOO_MANY, NO_TRIANGULATION = -1, 0, 1, 2
AREA_TOTALS = ("n_selected", "n_area_filled", "n_area_too_many_edges", "n_no_triangulation", "n_area_faces", "n_cells", "max_n")
AREA_INT_COLS = ("class", "n", "table_offset", "plan_face_offset", "row_offset", "face_offset")
WAVE_CANDIDATES = 64           # the device runs a cell with at least this many candidates as one wave: d - 1 >= 64
INF = np.float64(np.inf)


def weight(P, i, j, k, min_sin2):
    """T(i, j, k) on index arrays that broadcast"""
    with np.errstate(all="ignore"):
        a, b = P[j] - P[i], P[k] - P[i]
        g = b - a
        c = R._cross(a, b)
        n2, aa, bb, gg = R._dot(c, c), R._dot(a, a), R._dot(b, b), R._dot(g, g)
        e = np.where(bb > aa, bb, aa)
        e = np.where(gg > e, gg, e)
        return np.where(n2 > np.float64(min_sin2) * (e * e), np.float64(0.5) * np.sqrt(n2), INF)


def chord_mask(names, edges):
    """[n, n] bool: the chords (i, k), i < k, whose edge the table already holds, or whose names are equal"""
    n = len(names)
    i, k = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    chord = (i < k) & (k != i + 1) & ~((i == 0) & (k == n - 1))
    a, b = np.asarray(names, np.int64)[i], np.asarray(names, np.int64)[k]
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    have = np.isin(key, (e[:, 0] << 32) | e[:, 1])
    return chord & (have | (a == b))


def tables(P, forbidden, min_sin2):
    """(W float64 [n, n], J int32 [n, n]) of the loop with positions P (float64 [n, 3]); cells outside 0 <= i < k < n keep +inf, -1"""
    n = len(P)
    W, J = np.full((n, n), INF), np.full((n, n), -1, np.int32)
    r = np.arange(n - 1)
    W[r, r + 1] = 0.0
    with np.errstate(all="ignore"):
        for d in range(2, n):
            i = np.arange(n - d)
            k = i + d
            j = i[:, None] + 1 + np.arange(d - 1)[None]
            cand = (W[i[:, None], j] + W[j, k[:, None]]) + weight(P, i[:, None], j, k[:, None], min_sin2)
            a = np.argmin(cand, 1)                                                    # (the first of equal minima: the smallest j)
            W[i, k] = np.where(forbidden[i, k], INF, cand[i, a])
            J[i, k] = j[i, a]
    return W, J


def faces_of(J, loop_verts, base=0):
    """{number: (p_k, p_j, p_i)} in pre-order numbering from ``base``"""
    out, stack = {}, [(0, len(loop_verts) - 1, base)]
    while stack:
        i, k, b = stack.pop()
        if k - i < 2:
            continue
        j = int(J[i, k])
        assert i < j < k
        out[b] = (loop_verts[k], loop_verts[j], loop_verts[i])
        stack += [(i, j, b + 1), (j, k, b + 1 + (j - i - 1))]
    return out


def brute_force(P, forbidden, min_sin2):
    """(value, root j) of every cell (i, k) by enumeration of ALL triangulations of the sub-polygon, each evaluated by the nested
    expression (left + right) + T; the root is the smallest j among the triangulations of least value.  {(i, k): (value, j)}"""
    n = len(P)
    memo, best = {}, {}

    def trees(i, k):                                       # every (value, root j) of the sub-polygon i .. k
        if k == i + 1:
            return [(np.float64(0.0), -1)]
        if (i, k) not in memo:
            out = []
            for j in range(i + 1, k):
                t = weight(P, i, j, k, min_sin2)
                for vl, _ in blocked(i, j):
                    for vr, _ in blocked(j, k):
                        out.append(((vl + vr) + t, j))
            memo[(i, k)] = out
        return memo[(i, k)]

    def blocked(i, k):
        return [(INF if k > i + 1 and forbidden[i, k] else v, j) for v, j in trees(i, k)]

    for i in range(n):
        for k in range(i + 2, n):
            ts = trees(i, k)
            v = min(t[0] for t in ts)
            best[(i, k)] = (INF if forbidden[i, k] else v, min(j for w, j in ts if w == v))
    return best


def area_patches(verts, faces, tr, ints, class_mask, max_area_edges=2048, min_sin=1e-6, names=None):
    """Section 24 on a trace and loop table of fill_ref: dict with ``ints`` [L, 6], ``area`` [L], ``faces`` int64 [n_area_faces, 3]
    in the final numbering, ``totals``, ``tables`` {loop: (W, J, mask)}, the same laid out as the device's workspace (``W``, ``J``,
    ``mask`` [n_cells]: the tables of the loops in order, row-major), ``plan_faces`` (the plan's numbering: -1 rows for a loop
    without a triangulation) and ``n_rows``"""
    X = np.ascontiguousarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1)
    nm = f if names is None else np.asarray(names, np.int64).reshape(-1)
    edges = T.edge_table(nm.reshape(-1, 3), len(X))["edges"]
    min_sin2 = np.float64(min_sin) * np.float64(min_sin)
    L = len(ints)
    out, area, tabs, new, planned = np.zeros((L, 6), np.int64), np.zeros(L), {}, [], []
    cells = rows = plan_faces = final_faces = max_n = 0
    for l in range(L):
        n, s, c = int(ints[l, 1]), int(ints[l, 2]), int(ints[l, 3])
        cls = NOT_SELECTED if not (class_mask >> c) & 1 else AREA_TOO_MANY if n > max_area_edges else NO_TRIANGULATION if n < 3 \
            else AREA_FILLED
        out[l] = (cls, n, cells, plan_faces, rows, final_faces)
        if cls != AREA_FILLED:
            continue
        hs = tr["order"][s:s + n]
        mask = chord_mask(nm[hs], edges)
        W, J = tables(X[f[hs]], mask, min_sin2)
        tabs[l], area[l] = (W, J, mask), W[0, n - 1]
        cells, rows, plan_faces, max_n = cells + n * n, rows + n, plan_faces + n - 2, max(max_n, n)
        if np.isfinite(W[0, n - 1]):
            tri = faces_of(J, f[hs])
            new += [tri[b] for b in range(n - 2)]
            planned += [tri[b] for b in range(n - 2)]
            final_faces += n - 2
        else:
            out[l, 0] = NO_TRIANGULATION
            planned += [(-1, -1, -1)] * (n - 2)
    cls = out[:, 0]
    totals = dict(n_selected=int((cls >= 0).sum()), n_area_filled=int((cls == 0).sum()), n_area_too_many_edges=int((cls == 1).sum()),
                  n_no_triangulation=int((cls == 2).sum()), n_area_faces=final_faces, n_cells=cells, max_n=max_n)
    flat = [np.concatenate([tabs[l][c].reshape(-1) for l in sorted(tabs)]) if tabs else np.zeros(0, t) for c, t in
            enumerate((np.float64, np.int32, bool))]
    return dict(ints=out, area=area, faces=np.array(new, np.int64).reshape(-1, 3), totals=totals, tables=tabs, W=flat[0], J=flat[1],
                mask=flat[2], plan_faces=np.array(planned, np.int64).reshape(-1, 3), n_rows=rows)


def fill_holes(mesh, method="auto", max_area_edges=2048, min_sin=1e-6, names=None, **kw):
    """the statement of ``mesh_fill.fill_holes(method="auto" | "min_area")`` without fairing and normals: fill_ref.fill_holes' dict
    (the polar part; left out under "min_area") with the minimum-area faces appended and the keys ``area_ints``, ``area``,
    ``area_totals``, ``tables``, ``area_new_faces``"""
    assert method in ("auto", "min_area") and (method != "auto" or kw.get("skip_folded", True))
    ref = R.fill_holes(mesh, names=names, **kw)
    v32 = np.ascontiguousarray(mesh["verts"], np.float32).reshape(-1, 3)
    f = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    if method == "min_area":
        ref["verts"], ref["faces"], ref["new_vertex"] = v32, f.astype(np.int32), np.zeros(len(v32), bool)
        if "colors" in ref:
            ref["colors"] = np.ascontiguousarray(mesh["colors"], np.float32).reshape(-1, 3)
    a = area_patches(v32, f, ref["trace"], ref["ints"], 1 << R.FOLDED if method == "auto" else 1 << R.FILLED | 1 << R.FOLDED,
                     max_area_edges, min_sin, names)
    ref["faces"] = np.concatenate([ref["faces"], a["faces"].astype(np.int32)])
    ref.update(area_ints=a["ints"], area=a["area"], area_totals=a["totals"], tables=a["tables"], area_new_faces=a["faces"], patches=a)
    return ref


# ---- the meshes of the tests ----------------------------------------------------------------------------------------------------------

U_CELLS = [(2, 2), (3, 2), (4, 2), (4, 3), (4, 4), (3, 4), (2, 4)]


def mesh(v, f):
    return dict(verts=np.ascontiguousarray(v, np.float32), faces=np.ascontiguousarray(f, np.int32).reshape(-1, 3))


def u_grid():
    """grid_mesh(9) without a U of seven cells: loops [filled (32), folded (16)]; the U's patch has area exactly 7"""
    return mesh(*R.grid_without(9, U_CELLS))


def comb(n):
    """a planar sawtooth comb of n >= 5 points, counter-clockwise, integer coordinates (every sum is exact, ties abound)"""
    w = n - 3
    top = [(w - t, 4 if t % 2 == 0 else 1, 0) for t in range(n - 2)]
    return np.array([(0, 0, 0), (w, 0, 0)] + top, np.float32)


def spiral(n, turns=2.0):
    """a planar spiral arm of n >= 5 points: out along r = 0.5 + 0.25 theta, back along r - 0.6"""
    no = (n + 1) // 2
    th_o, th_i = np.linspace(0.0, 2 * np.pi * turns, no), np.linspace(2 * np.pi * turns, 0.0, n - no)
    ro, ri = 0.5 + 0.25 * th_o, 0.5 + 0.25 * th_i - 0.6 * (0.5 + 0.25 * th_i) / (0.5 + 0.25 * th_i).max() - 0.2
    x = np.concatenate([ro * np.cos(th_o), ri * np.cos(th_i)])
    y = np.concatenate([ro * np.sin(th_o), ri * np.sin(th_i)])
    return np.stack([x, y, np.zeros(n)], 1).astype(np.float32)


def noisy_ring(n, seed=5):
    """a non-planar ring r = 1 + 0.3 sin 7 theta with Gaussian z"""
    th = 2 * np.pi * np.arange(n) / n
    r = 1.0 + 0.3 * np.sin(7 * th)
    z = 0.1 * np.random.default_rng(seed).standard_normal(n)
    return np.stack([r * np.cos(th), r * np.sin(th), z], 1).astype(np.float32)


def collar(P, Q=None):
    """the closed polygon P [n, 3] and an offset copy Q of it (default: P moved down the z axis), joined by a band of faces.  The
    inner loop P is the hole; the outer loop has one vertex more (the midpoint of its last edge, 2 n + 1 faces in all), so that
    ``max_edges=n`` keeps it open."""
    P = np.asarray(P, np.float32)
    n = len(P)
    Q = P + np.array([0, 0, -1], np.float32) if Q is None else np.asarray(Q, np.float32)
    v = np.concatenate([P, Q, (0.5 * (Q[n - 1:n] + Q[0:1])).astype(np.float32)])
    f = []
    for i in range(n):
        i1 = (i + 1) % n
        f.append((i, i1, n + i1))
        f += [(i, n + i1, n + i)] if i < n - 1 else [(i, n, 2 * n), (i, 2 * n, n + i)]
    return mesh(v, f)


def shoelace(P):
    x, y = P[:, 0].astype(np.float64), P[:, 1].astype(np.float64)
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


COLLAR_SIZES = (5, 63, 64, 65, 66, 67, 129, 257)           # 65 | 66: the first loop with a one-wave diagonal (d - 1 = 64) is n = 66


def collar_cases():
    """{name: (mesh, keywords, planar polygon or None)}"""
    out = {}
    for n in COLLAR_SIZES:
        out[f"comb {n}"] = (collar(comb(n)), dict(max_edges=n), comb(n))
    for n in (64, 66, 129):
        out[f"spiral {n}"] = (collar(spiral(n)), dict(max_edges=n), spiral(n))
    for n in (5, 63, 65, 67, 257):
        P = noisy_ring(n)
        out[f"ring {n}"] = (collar(P, P * np.array([1.6, 1.6, 1.0], np.float32)), dict(max_edges=n), None)
    return out


def small_cases():
    """{name: (mesh, keywords)}: the smallest loops and the refusals"""
    import simplify_ref
    import smooth_ref
    line = simplify_ref.TET_V.copy()
    line[3] = 0.5 * (line[0] + line[2])                                                # the three loop vertices collinear
    f50, V50 = T.strip(50)
    return {
        "U grid": (u_grid(), {}),
        "U grid, small loops only": (u_grid(), dict(max_edges=16)),
        "open tetrahedron": (mesh(simplify_ref.TET_V, simplify_ref.TET_F[:3]), {}),
        "grid without one cell": (mesh(*R.grid_without(7, [(1, 1)])), dict(max_edges=4)),
        "grid of one cell": (mesh(*smooth_ref.grid_mesh(2)), {}),
        "grid with a hole": (mesh(*smooth_ref.grid_mesh(9, hole=(2, 3, 3))), dict(max_edges=12)),
        "collinear tetrahedron": (mesh(line, simplify_ref.TET_F[:3]), {}),
        "strip": (mesh(smooth_ref.index_only_mesh(f50, V50), f50), {}),
    }


def grid65():
    return mesh(*R.grid_without(65, [(4 * a + 1, 4 * b + 1) for a in range(16) for b in range(16)]))
