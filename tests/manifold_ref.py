"""Sequential numpy / Python restatement of header Section 26 (csrc/mesh_manifold.hip, nicer_slam_amd/mesh_repair.py) for
the tests: the fans of faces around every vertex, found through regular edges only on the edge table of tests/topology_ref.py, one
vertex per fan, and the inverse plumbing ``weld``.  Needs numpy (and topology_ref's scipy) only."""
import numpy as np

import topology_ref as T

TOTALS = ("n_contributing", "n_fans", "n_singular_verts", "n_pinch_only", "n_cut_edges", "n_new", "max_fans", "status")


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def _unite(parent, a, b):
    a, b = _find(parent, a), _find(parent, b)
    if a != b:
        parent[max(a, b)] = min(a, b)


def regular_edges(t, cut_inconsistent=False, labels=None):
    """bool [E]: count 2, (cut_inconsistent) traversed once each way, (labels) both faces of one label"""
    reg = t["edge_count"] == 2
    if cut_inconsistent:
        reg &= t["edge_forward"] == 1
    if labels is not None and len(reg):
        lab = np.asarray(labels).reshape(-1)
        s = np.minimum(t["edge_start"][:-1], max(len(t["edge_halfedges"]) - 2, 0))
        he = t["edge_halfedges"]
        same = np.zeros(len(reg), bool)
        two = t["edge_count"] == 2
        same[two] = lab[he[s[two]] // 3] == lab[he[s[two] + 1] // 3]
        reg &= same
    return reg


def split_fans(faces, n_verts, face_mask=None, cut_inconsistent=False, labels=None):
    """dict: corner_fan [3 F], vertex_fans [V], faces [F, 3], new_source [n_new] (all int64) and the totals of Section 26"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F, V = len(f), int(n_verts)
    H = 3 * F
    t = T.edge_table(f, V, face_mask)
    ok = t["face_edges"][:, 0] >= 0
    reg = regular_edges(t, cut_inconsistent, labels)
    cut = (t["edge_count"] >= 2) & ~reg
    flat = f.reshape(-1)
    parent = list(range(H))
    on_cut = np.zeros(V, bool)
    for e in range(t["n_edges"]):
        lo, hi = (int(x) for x in t["edges"][e])
        if cut[e]:
            on_cut[lo] = on_cut[hi] = True
        if not reg[e]:
            continue
        h0, h1 = (int(x) for x in t["edge_halfedges"][t["edge_start"][e]:t["edge_start"][e] + 2])
        at = lambda h, v: h if flat[h] == v else 3 * (h // 3) + (h % 3 + 1) % 3           # the corner of h's face at v, an end of h
        _unite(parent, at(h0, lo), at(h1, lo))
        _unite(parent, at(h0, hi), at(h1, hi))
    corner_fan = np.full(H, -1, np.int64)
    for c in range(H):
        if ok[c // 3]:
            corner_fan[c] = _find(parent, c)
    leaders = np.nonzero(corner_fan == np.arange(H))[0]                                  # ascending corner order
    leaders = leaders[np.argsort(flat[leaders], kind="stable")]                          # ascending (vertex, leader)
    lv = flat[leaders]
    head = np.ones(len(leaders), bool)
    head[1:] = lv[1:] != lv[:-1]
    r = np.cumsum(~head) - (~head)                                                       # exclusive scan of "not head of its run"
    name = np.where(head, lv, V + r)
    fan_name = np.full(H, -1, np.int64)
    fan_name[leaders] = name
    out = f.copy()
    out[~ok] = np.where(out[~ok] >= V, -1, out[~ok])
    oc = np.nonzero(np.repeat(ok, 3))[0]
    out.reshape(-1)[oc] = fan_name[corner_fan[oc]]
    vertex_fans = np.bincount(lv, minlength=V).astype(np.int64)
    sing = vertex_fans > 1
    return dict(corner_fan=corner_fan, vertex_fans=vertex_fans, faces=out, new_source=lv[~head].astype(np.int64),
                n_contributing=int(ok.sum()), n_fans=len(leaders), n_singular_verts=int(sing.sum()),
                n_pinch_only=int((sing & ~on_cut).sum()), n_cut_edges=int(cut.sum()), n_new=int((~head).sum()),
                max_fans=int(vertex_fans.max()) if V else 0, status=0)


def totals_of(r):
    return [int(r[k]) for k in TOTALS]


def fan_components(faces, n_verts, **kw):
    """(face_label [F], n): the contributing faces joined where they share a fan; the label is the smallest face index, -1 for a face
    that does not contribute"""
    r = split_fans(faces, n_verts, **kw)
    F = len(r["faces"])
    ok = r["corner_fan"].reshape(-1, 3)[:, 0] >= 0
    parent = list(range(F))
    first = {}
    for c in np.nonzero(r["corner_fan"] >= 0)[0]:
        fan = int(r["corner_fan"][c])
        _unite(parent, first.setdefault(fan, int(c) // 3), int(c) // 3)
    label = np.array([_find(parent, x) if ok[x] else -1 for x in range(F)], np.int64).reshape(-1)
    return label, int(np.unique(label[label >= 0]).size)


def weld(faces, names, n_verts):
    """(faces' [F', 3], representative [V'], n_dropped): vertex v is merged into the smallest index of its class of ``names`` [V]
    (welded names: equal for vertices to merge); the representatives that a kept face uses, ascending, are the new vertices; faces
    that no longer contribute are dropped"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = int(n_verts)
    names = np.asarray(names, np.int64).reshape(-1)
    rep_of_name = {}
    rep = np.zeros(V, np.int64)
    for v in range(V):
        rep[v] = rep_of_name.setdefault(int(names[v]), v)
    ok = ((f >= 0) & (f < V)).all(1)
    g = np.where(ok[:, None], rep[np.where(ok[:, None], f, 0)], -1)
    keep = ok & (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 2] != g[:, 0])
    used = np.unique(g[keep])
    new = np.full(V, -1, np.int64)
    new[used] = np.arange(len(used))
    return new[g[keep]].reshape(-1, 3), used, int((~keep).sum())


# ---- hand rows of DESIGN 4y ------------------------------------------------------------------------------------------------------

def bow_tie():
    return np.array([[0, 1, 2], [0, 3, 4]], np.int32), 5


def book():
    return np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32), 5


def vertex_star(n=300):
    """n triangles that share vertex 0 and nothing else: n fans at one vertex"""
    k = np.arange(n)
    return np.stack([np.zeros(n, np.int64), 2 * k + 1, 2 * k + 2], 1).astype(np.int32), 2 * n + 1


def hand_rows():
    """{name: (faces, V, faces', new_source)}"""
    return {"bow tie": bow_tie() + ([[0, 1, 2], [5, 3, 4]], [0]),
            "book": book() + ([[0, 1, 2], [7, 5, 3], [6, 8, 4]], [0, 0, 1, 1])}


def random_soup(rng, vmin=4, vmax=8, fmax=24):
    """(faces, V): up to ``fmax`` faces over V in [vmin, vmax] vertices, indices from -1 to V (both ends do not contribute)"""
    V = int(rng.integers(vmin, vmax + 1))
    F = int(rng.integers(0, fmax + 1))
    return rng.integers(-1, V + 1, size=(F, 3)).astype(np.int32), V


def concatenated_soups(n=200, seed=11):
    """n random soups over disjoint vertex ranges as one face list; an index -1 stays -1 and an index V of a soup becomes the total V,
    so the faces that do not contribute stay so"""
    rng = np.random.default_rng(seed)
    soups = [random_soup(rng) for _ in range(n)]
    total = sum(V for _, V in soups)
    out, base = [], 0
    for f, V in soups:
        g = f.astype(np.int64)
        out.append(np.where(g < 0, -1, np.where(g >= V, total, g + base)))
        base += V
    return np.concatenate(out).astype(np.int32), total


def clustered_torus(res=16, cell=0.45):
    """the marching-cubes torus of topology_ref clustered with simplify_ref (placement "mean"): (faces, V)"""
    import simplify_ref as S
    r = S.simplify(T.mc_mesh("torus", res), cell=cell, placement="mean")
    return np.asarray(r["faces"]).astype(np.int32), len(r["verts"])


def kernel_cases():
    """[(name, faces, V, keywords of split_fans)]: the smallest shapes at which the kernels (and the host rehearsal of their bodies) can
    go wrong -- the hand rows, runs of fans that span several waves and blocks, V on both sides of the radix pass counts, a mask,
    cut_inconsistent and labels"""
    rng = np.random.default_rng(7)
    out = [(name, f, V, {}) for name, (f, V, _, _) in hand_rows().items()]
    out += [("two tets sharing a vertex",) + T.two_tets_sharing_vertex() + ({},), ("two tets sharing an edge",) + T.two_tets_sharing_edge() + ({},),
            ("moebius",) + T.moebius(8) + ({},), ("moebius cut inconsistent",) + T.moebius(8) + (dict(cut_inconsistent=True),),
            ("fan 300",) + T.fan(300) + ({},), ("vertex star 300",) + vertex_star(300) + ({},), ("strip 5000",) + T.strip(5000) + ({},)]
    f, V = concatenated_soups(200)
    out += [("200 soups", f, V, {}), ("200 soups cut inconsistent", f, V, dict(cut_inconsistent=True)),
            ("200 soups labels", f, V, dict(labels=rng.integers(0, 3, len(f)).astype(np.int32))),
            ("200 soups mask", f, V, dict(face_mask=rng.integers(0, 2, len(f)).astype(np.uint8)))]
    for V in (255, 256, 257, 65535, 65536, 65537):
        f = np.concatenate([T.high_index_faces(V)[0], bow_tie()[0], bow_tie()[0] + (V - 5)]).astype(np.int32)
        out.append((f"high indices V {V}", f, V, {}))
    f, V = T.tetrahedron()
    out += [("labelled tetrahedron", f, V, dict(labels=np.array([0, 0, 1, 1], np.int32))),
            ("no vertices", np.array([[0, 1, 2], [-1, 0, 5]], np.int32), 0, {})]
    return out
