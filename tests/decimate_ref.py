"""numpy restatement of header Section 22 (csrc/mesh_decimate.hip, csrc/decimate_passes.hpp, nicer_slam_amd/mesh_decimate.py)
for the tests: edge-collapse decimation with quadric error in rounds of independent collapses, float64 with one numpy operation per
rounded operation of the statement.  Vectorised over edges, (edge, neighbour) and (edge, face) pairs; ordered sums run over the columns
of a padded matrix as in smooth_ref.  The mesh makers come from simplify_ref, topology_ref, smooth_ref and clean_ref unchanged.  Needs
numpy and scipy (through topology_ref) only."""
import numpy as np

import clean_ref          # noqa: F401  (adversarial_cases, for the tests)
import simplify_ref       # noqa: F401  (icosphere, cube, adversarial_mesh, volume, cube_surface_distance)
import smooth_ref as S
import topology_ref as T

BOUNDARY = ("quadric", "fixed")
CANDIDATE, REJ_LOCK, REJ_ERROR, REJ_LINK, REJ_FOLD = 0, 1, 2, 3, 4
TOTALS = ("rounds", "collapses", "n_candidates", "rej_lock", "rej_error", "rej_link", "rej_fold", "n_selected", "n_faces", "n_verts",
          "status")
BIG = np.iinfo(np.int64).max


def _dot(u, w):
    return (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]


def _cross(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                     u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def _normal(p0, p1, p2):
    return _cross(p1 - p0, p2 - p0)


def _plane_terms(n, p, s=None):
    """[m, 11]: s * (n n^T (6), n d (3), d^2, n . n) with d = -(n . p); unscaled when s is None"""
    d = -_dot(n, p)
    sn = n if s is None else s[:, None] * n
    sd = d if s is None else s * d
    nn = _dot(n, n)
    return np.stack([sn[:, 0] * n[:, 0], sn[:, 0] * n[:, 1], sn[:, 0] * n[:, 2], sn[:, 1] * n[:, 1], sn[:, 1] * n[:, 2],
                     sn[:, 2] * n[:, 2], sn[:, 0] * d, sn[:, 1] * d, sn[:, 2] * d, sd * d, nn if s is None else s * nn], 1)


def _finite_faces(X, f):
    ok = T.contributing(f, len(X))
    ok[ok] = np.isfinite(X[f[ok]]).all(2).all(1)
    return ok


class State:
    """the state between rounds: X [V, 3], Q [V, 11], C [V, 3] or None (float64), faces [F, 3] int64, vmap [V], locked, moved [V]"""

    def __init__(self, verts, faces, colors=None, fixed=None, boundary="quadric", boundary_weight=1.0):
        assert boundary in BOUNDARY
        self.v32 = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        self.c32 = None if colors is None else np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
        self.X = self.v32.astype(np.float64)
        self.C = None if colors is None else self.c32.astype(np.float64)
        self.faces = np.asarray(faces, np.int64).reshape(-1, 3).copy()
        V = self.V = len(self.X)
        self.vmap = np.arange(V)
        self.moved = np.zeros(V, bool)
        self.log = []
        X, f = self.X, self.faces
        table, ring = self.tables()
        with np.errstate(all="ignore"):
            # face terms at the corners, ascending corner id
            ok = _finite_faces(X, f)
            g = np.nonzero(ok)[0]
            fn = _normal(X[f[g, 0]], X[f[g, 1]], X[f[g, 2]])
            ft = _plane_terms(fn, X[f[g, 0]])
            c_vert = f[g].reshape(-1)                                                     # corner 3 g + k, ascending
            c_term = np.repeat(ft, 3, 0)
            order = np.argsort(c_vert, kind="stable")
            owner_f, term_f = c_vert[order], c_term[order]
            # boundary terms along the rows, ascending neighbour
            start, nbr, eid = ring["ring_start"], ring["ring"], ring["ring_edge"]
            owner = S._owners(start)
            cnt = table["edge_count"][eid] if len(eid) else np.zeros(0, np.int64)
            finite_v = np.isfinite(X).all(1)
            locked = ~finite_v
            if fixed is not None:
                locked |= np.asarray(fixed).reshape(-1) != 0
            bad = ~finite_v[nbr] | (cnt > 2) | ((cnt == 1) if boundary == "fixed" else np.zeros(len(cnt), bool))
            locked[owner[bad]] = True
            b = np.nonzero(cnt == 1)[0]
            bg = table["edge_halfedges"][table["edge_start"][eid[b]]] // 3 if len(b) else np.zeros(0, np.int64)
            keep = ok[bg]
            b, bg = b[keep], bg[keep]
            lo, hi = np.minimum(owner[b], nbr[b]), np.maximum(owner[b], nbr[b])
            n = _normal(X[f[bg, 0]], X[f[bg, 1]], X[f[bg, 2]])
            ev = X[hi] - X[lo]
            m = _cross(ev, n)
            ee = _dot(ev, ev)
            sc = np.float64(boundary_weight) / ee
            keep = (ee > 0.0) & np.isfinite(sc)
            bt = _plane_terms(m[keep], X[lo[keep]], sc[keep])
            owner_b = owner[b[keep]]
            # per vertex: the face terms, then the boundary terms
            own = np.concatenate([owner_f, owner_b])
            term = np.concatenate([term_f, bt])
            o2 = np.argsort(own, kind="stable")
            M, count = S._padded(own[o2], term[o2], V)
            Q = np.zeros((V, 11))
            for j in range(M.shape[1]):
                Q = np.where((j < count)[:, None], Q + M[:, j], Q)
        self.Q, self.locked, self.Q0 = Q, locked, Q.copy()

    def tables(self):
        table = T.edge_table(self.faces, self.V)
        return table, S.vertex_ring(self.faces, self.V, table)

    def n_faces(self):
        return int(T.contributing(self.faces, self.V).sum())


def place_and_cost(q, a, b, eps):
    """(x [m, 3], cost [m], finite cost [m]) of the summed quadrics q [m, 11] between the ends a, b"""
    with np.errstate(all="ignore"):
        m = (a + b) * 0.5
        tr = (q[:, 0] + q[:, 3]) + q[:, 5]
        mu = np.float64(eps) * tr
        a00, a11, a22, a01, a02, a12 = q[:, 0] + mu, q[:, 3] + mu, q[:, 5] + mu, q[:, 1], q[:, 2], q[:, 4]
        r0, r1, r2 = mu * m[:, 0] - q[:, 6], mu * m[:, 1] - q[:, 7], mu * m[:, 2] - q[:, 8]
        d0 = a00
        l10, l20 = a01 / d0, a02 / d0
        d1 = a11 - l10 * a01
        t = a12 - l20 * a01
        l21 = t / d1
        d2 = (a22 - l20 * a02) - l21 * t
        y0 = r0
        y1 = r1 - l10 * y0
        y2 = (r2 - l20 * y0) - l21 * y1
        x2 = y2 / d2
        x1 = y1 / d1 - l21 * x2
        x0 = (y0 / d0 - l10 * x1) - l20 * x2
        xs = np.stack([x0, x1, x2], 1)
        solved = (tr != 0.0) & np.isfinite(tr) & (d0 > 0.0) & (d1 > 0.0) & (d2 > 0.0) & np.isfinite(xs).all(1)
        x = np.where(solved[:, None], xs, m)
        ax0 = (q[:, 0] * x[:, 0] + q[:, 1] * x[:, 1]) + q[:, 2] * x[:, 2]
        ax1 = (q[:, 1] * x[:, 0] + q[:, 3] * x[:, 1]) + q[:, 4] * x[:, 2]
        ax2 = (q[:, 2] * x[:, 0] + q[:, 4] * x[:, 1]) + q[:, 5] * x[:, 2]
        xax = (x[:, 0] * ax0 + x[:, 1] * ax1) + x[:, 2] * ax2
        bx = (q[:, 6] * x[:, 0] + q[:, 7] * x[:, 1]) + q[:, 8] * x[:, 2]
        c = (xax + 2.0 * bx) + q[:, 9]
        fin = np.isfinite(c)
        return x, np.where(c > 0.0, c, 0.0), fin


def _fold_fails(st, table, lo, hi, x, min_cos2):
    """bool [E]: some face around lo or hi that does not hold both turns over or loses its shape with that end at x"""
    f, X, V = st.faces, st.X, st.V
    E = len(lo)
    g = np.nonzero(T.contributing(f, V))[0]
    inc_v = f[g].reshape(-1)
    inc_g = np.repeat(g, 3)
    order = np.argsort(inc_v, kind="stable")
    inc_v, inc_g = inc_v[order], inc_g[order]
    first = np.searchsorted(inc_v, np.arange(V + 1))
    fails = np.zeros(E, bool)
    with np.errstate(all="ignore"):
        for end, other in ((lo, hi), (hi, lo)):
            n_inc = first[end + 1] - first[end]
            e_of = np.repeat(np.arange(E), n_inc)
            pos = np.arange(len(e_of)) - np.repeat(np.cumsum(n_inc) - n_inc, n_inc) + np.repeat(first[end], n_inc)
            gg = inc_g[pos]
            tri = f[gg]
            keep = ~(tri == other[e_of][:, None]).any(1)
            e_of, tri = e_of[keep], tri[keep]
            P = X[tri]                                                                    # [m, 3, 3]
            P2 = np.where((tri == end[e_of][:, None])[:, :, None], x[e_of][:, None, :], P)
            n = _normal(P[:, 0], P[:, 1], P[:, 2])
            n2 = _normal(P2[:, 0], P2[:, 1], P2[:, 2])
            d, nn, mm = _dot(n, n2), _dot(n, n), _dot(n2, n2)
            bad = ~(d > 0.0) | ~(d * d > (np.float64(min_cos2) * nn) * mm)
            fails[e_of[bad]] = True
    return fails


def evaluate(st, table, ring, eps=1e-3, max_error=None, min_cos=0.2):
    """(code [E], cost [E] float64, place [E, 3]): every edge of the table through lock, placement and error, link, fold, in that order"""
    e = table["edges"].reshape(-1, 2)
    E, V = len(e), st.V
    lo, hi = e[:, 0], e[:, 1]
    cnt = table["edge_count"]
    code = np.full(E, -1, np.int64)
    code[st.locked[lo] | st.locked[hi] | (cnt < 1) | (cnt > 2)] = REJ_LOCK
    q = st.Q[lo] + st.Q[hi]
    x, cost, fin = place_and_cost(q, st.X[lo], st.X[hi], eps)
    err = ~fin
    if max_error is not None:
        me2 = np.float64(max_error) * np.float64(max_error)
        with np.errstate(all="ignore"):
            err |= ~(cost <= me2 * q[:, 10])
    code[(code < 0) & err] = REJ_ERROR
    # the link
    start, nbr, eid = ring["ring_start"], ring["ring"], ring["ring_edge"]
    deg = np.diff(start)
    owner = S._owners(start)
    onb = np.zeros(V, bool)
    onb[owner[cnt[eid] == 1]] = True
    keys = (lo << 32) | hi
    n_lo = deg[lo]
    e_of = np.repeat(np.arange(E), n_lo)
    at = np.arange(len(e_of)) - np.repeat(np.cumsum(n_lo) - n_lo, n_lo) + np.repeat(start[lo], n_lo)
    u = nbr[at]
    h = hi[e_of]
    k = (np.minimum(u, h) << 32) | np.maximum(u, h)
    p = np.searchsorted(keys, k)
    found = (u != h) & (p < E) & (keys[np.minimum(p, max(E - 1, 0))] == k) if E else np.zeros(0, bool)
    common = np.bincount(e_of[found], minlength=E)
    virt = (cnt == 2) & onb[lo] & onb[hi]
    merged = deg[lo] + deg[hi] - common
    link = (common + virt == cnt) & (merged >= np.where(cnt == 1, 4, 5))
    code[(code < 0) & ~link] = REJ_LINK
    open_ = np.nonzero(code < 0)[0]                                                       # (only the edges still undecided: a hub's row is long)
    fold = _fold_fails(st, table, lo[open_], hi[open_], x[open_], np.float64(min_cos) * np.float64(min_cos))
    code[open_[fold]] = REJ_FOLD
    code[code < 0] = CANDIDATE
    return code, cost, x


def mix64(w):
    """the key's second word: splitmix64's finaliser of lo << 32 | hi, a bijection of the 64-bit words (uint64 arithmetic wraps)"""
    z = w + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def select(code, cost, table, ring, V):
    """the selected edge ids in key order: (cost bits, mix64(lo << 32 | hi))"""
    E = len(code)
    e = table["edges"].reshape(-1, 2)
    bits = np.ascontiguousarray(cost, np.float64).view(np.uint64)
    word = mix64((e[:, 0].astype(np.uint64) << np.uint64(32)) | e[:, 1].astype(np.uint64))
    cand = code == CANDIDATE
    rank = np.full(E, BIG, np.int64)
    ids = np.nonzero(cand)[0]
    order = ids[np.lexsort((word[ids], bits[ids]))]
    rank[order] = np.arange(len(order))
    start, nbr, eid = ring["ring_start"], ring["ring"], ring["ring_edge"]
    owner = S._owners(start)
    m1 = np.full(V, BIG, np.int64)
    np.minimum.at(m1, owner, rank[eid])
    m2 = m1.copy()
    np.minimum.at(m2, owner, m1[nbr])
    sel = cand & (m2[e[:, 0]] == rank) & (m2[e[:, 1]] == rank)
    ids = np.nonzero(sel)[0]
    return ids[np.argsort(rank[ids])]


def prefix(sel, edge_count, n_faces, target):
    """the shortest prefix of the selected edges (in key order) that brings the face count to <= target; all of them without a target"""
    if target is None:
        return sel
    ec = edge_count[sel]
    before = np.cumsum(ec) - ec
    return sel[n_faces - before > target]


def apply(st, table, taken, cost, x, rnd):
    e = table["edges"].reshape(-1, 2)
    lo, hi = e[taken, 0], e[taken, 1]
    X, V = st.X, st.V
    with np.errstate(all="ignore"):
        if st.C is not None:
            ev, dx = X[hi] - X[lo], x[taken] - X[lo]
            ee = _dot(ev, ev)
            t = np.where(ee > 0.0, _dot(dx, ev) / np.where(ee > 0.0, ee, 1.0), 0.0)
            t = np.where(t > 0.0, t, 0.0)
            t = np.where(t < 1.0, t, 1.0)
            st.C[lo] = st.C[lo] + t[:, None] * (st.C[hi] - st.C[lo])
        X[lo] = x[taken]
        st.Q[lo] = st.Q[lo] + st.Q[hi]
    st.vmap[hi] = lo
    st.moved[lo] = True
    bits = np.ascontiguousarray(cost[taken], np.float64).view(np.uint64)
    st.log += [(rnd, int(a), int(b), int(c)) for a, b, c in zip(lo, hi, bits)]
    f = st.faces
    ok = (f >= 0) & (f < V)
    st.faces = np.where(ok, st.vmap[np.where(ok, f, 0)], f)
    r = st.vmap
    st.vmap = np.where(r[r] != r, r[r], r)


def run_round(st, rnd, target_faces=None, max_error=None, min_cos=0.2, eps=1e-3, only=None):
    """one round on ``st``; returns a dict of the round's totals.  ``only`` = (lo, hi): that edge alone is collapsed (it must be a
    candidate), for replaying a round one collapse at a time"""
    table, ring = st.tables()
    code, cost, x = evaluate(st, table, ring, eps, max_error, min_cos)
    n_faces = table["n_contributing"]
    if only is None:
        sel = select(code, cost, table, ring, st.V)
        taken = prefix(sel, table["edge_count"], n_faces, target_faces)
    else:
        e = table["edges"].reshape(-1, 2)
        sel = taken = np.nonzero((e[:, 0] == only[0]) & (e[:, 1] == only[1]) & (code == CANDIDATE))[0]
        assert len(taken) == 1, "the edge is no candidate any more"
    removed = int(table["edge_count"][taken].sum())
    apply(st, table, taken, cost, x, rnd)
    return dict(n_candidates=int((code == CANDIDATE).sum()), rej_lock=int((code == REJ_LOCK).sum()),
                rej_error=int((code == REJ_ERROR).sum()), rej_link=int((code == REJ_LINK).sum()),
                rej_fold=int((code == REJ_FOLD).sum()), n_selected=len(sel), n_taken=len(taken), n_faces=n_faces - removed,
                selected=sel, edges=table["edges"].reshape(-1, 2), ring=ring)


def finish(st, normals="angle"):
    V = st.V
    ok = T.contributing(st.faces, V)
    face_origin = np.nonzero(ok)[0]
    used = np.zeros(V, bool)
    used[st.faces[ok].reshape(-1)] = True
    new = np.cumsum(used) - 1
    verts = st.v32.copy()
    verts[st.moved] = st.X[st.moved].astype(np.float32)
    out = dict(verts=verts[used], faces=new[st.faces[ok]].astype(np.int32).reshape(-1, 3))
    if st.C is not None:
        col = st.c32.copy()
        col[st.moved] = st.C[st.moved].astype(np.float32)
        out["colors"] = col[used]
    if normals is not None:
        out["normals"] = S.vertex_normals(out["verts"], out["faces"], normals)
    out["vertex_map"] = np.where(used[st.vmap], new[st.vmap], -1).astype(np.int32)
    out["face_origin"] = face_origin.astype(np.int32)
    out["log"] = np.array(st.log, np.uint64).reshape(-1, 4)
    return out


def decimate(mesh, target_faces=None, max_error=None, boundary="quadric", boundary_weight=1.0, min_cos=0.2, eps=1e-3, fixed=None,
             max_rounds=256, normals="angle", rounds_out=None):
    """the statement of ``mesh_decimate.decimate(..., return_map=True)`` on numpy arrays.  ``rounds_out``: a list that receives every
    round's dict.  The result also carries the final ``state``"""
    assert target_faces is not None or max_error is not None
    st = State(mesh["verts"], mesh["faces"], mesh.get("colors"), fixed, boundary, boundary_weight)
    last = dict.fromkeys(("n_candidates", "rej_lock", "rej_error", "rej_link", "rej_fold", "n_selected"), 0)
    n_faces, rounds = st.n_faces(), 0
    while rounds < max_rounds and n_faces > 0 and st.V > 0:
        if target_faces is not None and n_faces <= target_faces:
            break
        r = run_round(st, rounds, target_faces, max_error, min_cos, eps)
        rounds += 1
        n_faces = r["n_faces"]
        last = {k: r[k] for k in last}
        if rounds_out is not None:
            rounds_out.append(r)
        if r["n_taken"] == 0:
            break
    out = finish(st, normals)
    out["state"] = st
    out["totals"] = dict(rounds=rounds, collapses=len(st.log), **last, n_faces=len(out["faces"]), n_verts=len(out["verts"]), status=0)
    return out


# ---- meshes and measures --------------------------------------------------------------------------------------------------------------

def mesh_of(verts, faces, colors=False, seed=3):
    m = dict(verts=np.ascontiguousarray(verts, np.float32), faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3))
    if colors:
        m["colors"] = np.random.default_rng(seed).random((len(m["verts"]), 3)).astype(np.float32)
    return m


def area(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    return float(0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum())


def surface_samples(verts, faces, per_face=1, seed=0):
    """area-weighted random points on a mesh (for two-sided distances): n_faces * per_face points"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    g = np.random.default_rng(seed)
    a = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    pick = g.choice(len(f), size=max(len(f) * per_face, 2000), p=a / a.sum())
    r1, r2 = np.sqrt(g.random(len(pick))), g.random(len(pick))
    w = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], 1)
    return (v[f[pick]] * w[:, :, None]).sum(1)
