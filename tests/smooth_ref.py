"""numpy restatement of header Section 21 (csrc/mesh_smooth.hip, nicer_slam_amd/mesh_smooth.py) for the tests: the vertex
rings from ``topology_ref.edge_table``, the smoothing steps and the vertex normals in float64 with one numpy operation per rounded
operation of the statement, and the meshes the tests use.  Vectorised: a padded neighbour (or corner) matrix and a loop over its
columns with ``np.where``, never over vertices.  Needs numpy and scipy (through topology_ref) only."""
import numpy as np

import simplify_ref
import topology_ref as T

BOUNDARY = ("free", "fixed", "curve")
LIVE, ON_BOUNDARY, MOVES, STEPS = 1, 2, 4, 8


# ---- the vertex ring ------------------------------------------------------------------------------------------------------------------

def vertex_ring(faces, n_verts, table=None):
    """dict: ring_start [V + 1], ring [2 E], ring_edge [2 E] -- row v lists every u with {u, v} an edge, in ascending u -- and the
    edge table they came from as ``table``"""
    t = table or T.edge_table(faces, n_verts)
    e, V = t["edges"], int(n_verts)
    E = len(e)
    owner = np.concatenate([e[:, 0], e[:, 1]]).astype(np.int64)
    nbr = np.concatenate([e[:, 1], e[:, 0]]).astype(np.int64)
    eid = np.concatenate([np.arange(E), np.arange(E)])
    order = np.lexsort((nbr, owner))                                     # by owner, then by neighbour (an edge is listed once)
    start = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=V))]).astype(np.int64)
    return dict(ring_start=start, ring=nbr[order], ring_edge=eid[order], table=t)


def _owners(start):
    return np.repeat(np.arange(len(start) - 1), np.diff(start))


def _padded(owner, values, n_rows):
    """(matrix [n_rows, K] of ``values`` row by row in their order, zero padded; count [n_rows]); ``owner`` ascending"""
    count = np.bincount(owner, minlength=n_rows)
    K = int(count.max()) if len(owner) else 0
    first = np.concatenate([[0], np.cumsum(count)])[:-1]
    M = np.zeros((n_rows, max(K, 1)) + values.shape[1:], values.dtype)
    M[owner, np.arange(len(owner)) - first[owner]] = values
    return M, count


# ---- smoothing ------------------------------------------------------------------------------------------------------------------------

def smooth_state(verts, ring, boundary="curve", fixed=None):
    """(state [V] uint8: 1 live | 2 on_boundary | 4 moves | 8 moves with |N'| > 0, NB [V, K] the padded N' in row order, n [V])"""
    assert boundary in BOUNDARY
    X0 = np.asarray(verts, np.float32).astype(np.float64)
    V = len(X0)
    start, nbr, eid = ring["ring_start"], ring["ring"], ring["ring_edge"]
    owner = _owners(start)
    on_edge = ring["table"]["edge_count"][eid] == 1 if len(eid) else np.zeros(0, bool)
    live = np.isfinite(X0).all(1) & (np.diff(start) > 0)
    on_b = np.zeros(V, bool)
    on_b[owner[on_edge]] = True
    held = np.zeros(V, bool) if fixed is None else np.asarray(fixed).reshape(-1) != 0
    moves = live & ~held & ~(on_b if boundary == "fixed" else np.zeros(V, bool))
    member = moves[owner] & live[nbr]
    if boundary == "curve":
        member &= ~on_b[owner] | on_edge
    NB, n = _padded(owner[member], nbr[member], V)
    state = live * LIVE + on_b * ON_BOUNDARY + moves * MOVES + (n > 0) * STEPS
    return state.astype(np.uint8), NB, n


def smooth_steps(verts, faces, factors, boundary="curve", fixed=None, max_move=None, ring=None):
    """(out float32 [V, 3], state uint8 [V]): the statement of nsa_mesh_smooth.  Float64 positions between the steps; a vertex
    that cannot move keeps its input bits."""
    v32 = np.ascontiguousarray(verts, np.float32)
    ring = ring or vertex_ring(faces, len(v32))
    state, NB, n = smooth_state(v32, ring, boundary, fixed)
    steps = n > 0
    X0 = v32.astype(np.float64)
    X = X0.copy()
    nn = np.maximum(n, 1).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        for f in factors:
            assert abs(f) <= 1.0
            S = X[NB[:, 0]]
            for j in range(1, NB.shape[1]):
                S = np.where((j < n)[:, None], S + X[NB[:, j]], S)
            m = S / nn
            d = m - X
            Y = X + np.float64(f) * d
            if max_move is not None and np.isfinite(max_move):
                Y = np.minimum(np.maximum(Y, X0 - np.float64(max_move)), X0 + np.float64(max_move))
            X = np.where(steps[:, None], Y, X)
    out = v32.copy()
    if len(factors):
        out[steps] = X[steps].astype(np.float32)
    return out, state


def factors_of(method="taubin", iterations=10, lam=0.5, mu=-0.53):
    return [lam] * iterations if method == "laplacian" else [lam, mu] * iterations


# ---- vertex normals -------------------------------------------------------------------------------------------------------------------

def vertex_normals(verts, faces, weighting="area", return_sums=False):
    """float32 [V, 3]: the statement of nsa_mesh_vertex_normals.  ``return_sums``: also N [V, 3] float64, the sum of the weights
    (theta, or |n|) [V] and the corner count [V]"""
    assert weighting in ("area", "angle")
    v32 = np.ascontiguousarray(verts, np.float32)
    X = v32.astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(X)
    ok = T.contributing(f, V)
    ok[ok] = np.isfinite(X[f[ok]]).all(2).all(1)
    g = f[ok]
    c = (3 * np.nonzero(ok)[0][:, None] + np.arange(3)[None]).reshape(-1)             # corner ids, ascending
    k = c % 3
    rows = np.repeat(np.arange(len(g)), 3)
    p0, p1, p2 = X[g[rows, k]], X[g[rows, (k + 1) % 3]], X[g[rows, (k + 2) % 3]]
    with np.errstate(all="ignore"):
        a, b = p1 - p0, p2 - p0
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        if weighting == "angle":
            theta = np.arctan2(ln, (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])
            keep = ln > 0.0
            term, weight = (theta[:, None] * (n / ln[:, None]))[keep], theta[keep]
        else:
            keep = np.ones(len(c), bool)
            term, weight = n, ln
        vert = g[rows, k][keep]
        order = np.argsort(vert, kind="stable")                                       # ascending corner id within a vertex
        M, count = _padded(vert[order], term[order], V)
        N = np.zeros((V, 3))
        for j in range(M.shape[1]):
            N = np.where((j < count)[:, None], N + M[:, j], N)
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        good = (length > 0.0) & np.isfinite(length)
        out = np.where(good[:, None], N / np.where(good, length, 1.0)[:, None], 0.0).astype(np.float32)
    if return_sums:
        return out, N, np.bincount(vert, weights=weight, minlength=V), count
    return out


# ---- meshes and measures --------------------------------------------------------------------------------------------------------------

def noisy_icosphere(subdivisions, noise=0.02, seed=5):
    """(verts float32, faces int32, clean verts float32): the unit icosphere with every vertex moved along its radius by a normal
    deviate of standard deviation ``noise``"""
    v, f = simplify_ref.icosphere(subdivisions)
    r = 1.0 + noise * np.random.default_rng(seed).standard_normal(len(v))
    return (v.astype(np.float64) * r[:, None]).astype(np.float32), f, v


def rms_radial_error(verts):
    return float(np.sqrt(np.mean((np.linalg.norm(np.asarray(verts, np.float64), axis=1) - 1.0) ** 2)))


def volume(verts, faces):
    return simplify_ref.volume(verts, faces)


def grid_mesh(n=17, hole=None, heights=0.0, seed=2):
    """(verts float32 [n * n, 3], faces int32): an n x n lattice of unit cells split along one diagonal, z = ``heights`` times uniform
    deviates; ``hole`` = (i0, j0, m) leaves out the m x m cells from cell (i0, j0)"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    z = heights * np.random.default_rng(seed).uniform(-1.0, 1.0, (n, n)) + 0.0        # (+ 0.0: no negative zero in a flat grid)
    v = np.stack([i, j, z], 2).reshape(-1, 3).astype(np.float32)
    ci, cj = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    ci, cj = ci.reshape(-1), cj.reshape(-1)
    if hole is not None:
        i0, j0, m = hole
        keep = ~((ci >= i0) & (ci < i0 + m) & (cj >= j0) & (cj < j0 + m))
        ci, cj = ci[keep], cj[keep]
    a, b, c, d = ci * n + cj, (ci + 1) * n + cj, (ci + 1) * n + cj + 1, ci * n + cj + 1
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return v, f.astype(np.int32)


def fan_mesh(n=300, seed=4):
    """topology_ref.fan(n) with coordinates: the two hub vertices on the z axis, the others at random radii around it"""
    f, V = T.fan(n)
    g = np.random.default_rng(seed)
    ang = g.uniform(0.0, 2.0 * np.pi, V)
    rad = g.uniform(0.5, 1.5, V)
    v = np.stack([rad * np.cos(ang), rad * np.sin(ang), g.uniform(-0.2, 0.2, V)], 1)
    v[0], v[1] = (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)
    return v.astype(np.float32), f


def index_only_mesh(faces, V, seed=9):
    """finite random coordinates for an index-only face list"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (V, 3)).astype(np.float32)
