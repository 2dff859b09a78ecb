"""numpy restatement of header Section 18 (csrc/mesh_topology.hip, nicer_slam_amd/mesh_topology.py) for the tests: the
undirected edge table by ``np.unique`` on int64 keys, its classes and totals, boundary loops and edge-joined face components by
``scipy.sparse.csgraph.connected_components`` canonicalised to the smallest index, and the hand-derivable meshes the tests use.
Needs numpy and scipy only."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def contributing(faces, n_verts, face_mask=None):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < n_verts)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    if face_mask is not None:
        ok &= np.asarray(face_mask).reshape(-1) != 0
    return ok


def _smallest_index_labels(n, a, b, nodes):
    """label [n]: the smallest index of the component of the graph with edges (a[i], b[i]); -1 outside ``nodes`` (bool [n])"""
    label = np.full(n, -1, np.int64)
    if n == 0 or not nodes.any():
        return label
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    idx = np.nonzero(nodes)[0]
    smallest = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(smallest, comp[idx], idx)
    label[idx] = smallest[comp[idx]]
    return label


def edge_table(faces, n_verts, face_mask=None):
    """dict: edges [E, 2], edge_count [E], edge_forward [E], edge_start [E + 1], edge_halfedges [H_c], face_edges [F, 3] and the
    totals n_edges, n_contributing, n_used_verts, n_boundary, n_nonmanifold, n_inconsistent, n_boundary_loops."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F, V = len(f), int(n_verts)
    ok = contributing(f, V, face_mask)
    h = (3 * np.nonzero(ok)[0][:, None] + np.arange(3)[None]).reshape(-1)               # contributing half-edge ids, ascending
    a, b = f[h // 3, h % 3], f[h // 3, (h % 3 + 1) % 3]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = (lo << 32) | hi
    ukey, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    E = len(ukey)
    edges = np.stack([ukey >> 32, ukey & 0xFFFFFFFF], 1).reshape(-1, 2)
    forward = np.bincount(inv[a < b], minlength=E)
    order = np.argsort(inv, kind="stable")                                               # ascending half-edge id within an edge
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    face_edges = np.full((F, 3), -1, np.int64)
    face_edges.reshape(-1)[h] = inv
    bnd = count == 1
    # boundary loops: components of the boundary edges' graph, over the vertices they touch
    on = np.zeros(V, bool)
    on[edges[bnd].reshape(-1)] = True
    vl = _smallest_index_labels(V, edges[bnd, 0], edges[bnd, 1], on)
    return dict(edges=edges, edge_count=count.astype(np.int64), edge_forward=forward.astype(np.int64), edge_start=start,
                edge_halfedges=h[order], face_edges=face_edges, n_edges=E, n_contributing=int(ok.sum()),
                n_used_verts=int(np.unique(f[ok]).size), n_boundary=int(bnd.sum()), n_nonmanifold=int((count > 2).sum()),
                n_inconsistent=int(((count == 2) & (forward != 1)).sum()), n_boundary_loops=int(np.unique(vl[vl >= 0]).size))


def face_components(faces, n_verts, face_mask=None, table=None):
    """(face_label [F], n_components): faces that share an edge of any count >= 2 are joined; the label is the smallest face index"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    t = table or edge_table(f, n_verts, face_mask)
    he, start = t["edge_halfedges"], t["edge_start"]
    pos = np.arange(len(he))
    later = np.ones(len(he), bool)
    later[start[:-1]] = False                                                            # every half-edge of a run after the first
    label = _smallest_index_labels(len(f), he[pos[later]] // 3, he[pos[later] - 1] // 3, t["face_edges"][:, 0] >= 0)
    return label, int(np.unique(label[label >= 0]).size)


def face_adjacency(faces, n_verts, table=None):
    """[P, 2]: the face pairs of the edges with exactly two faces, f0 < f1, in edge order (trimesh's face_adjacency)"""
    t = table or edge_table(faces, n_verts)
    s = t["edge_start"][:-1][t["edge_count"] == 2]
    return np.stack([t["edge_halfedges"][s] // 3, t["edge_halfedges"][s + 1] // 3], 1).reshape(-1, 2)


def topology(faces, n_verts, face_mask=None):
    t = edge_table(faces, n_verts, face_mask)
    _, C = face_components(faces, n_verts, face_mask, t)
    r = {k: t[k] for k in ("n_contributing", "n_used_verts", "n_edges", "n_boundary", "n_nonmanifold", "n_inconsistent",
                           "n_boundary_loops")}
    r["n_faces"] = len(np.asarray(faces).reshape(-1, 3))
    r["n_components"] = C
    r["euler"] = r["n_used_verts"] - r["n_edges"] + r["n_contributing"]
    r["is_watertight"] = r["n_contributing"] > 0 and r["n_boundary"] == 0 and r["n_nonmanifold"] == 0
    r["is_oriented"] = r["is_watertight"] and r["n_inconsistent"] == 0
    return r


# ---- meshes whose answers can be derived by hand ------------------------------------------------------------------------------------

TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)                  # outward for a positively oriented (0, 1, 2, 3)


def tetrahedron():
    return TET.copy(), 4


def tetrahedron_one_reversed():
    f = TET.copy()
    f[2] = f[2, ::-1]
    return f, 4


def two_tets_sharing_vertex():
    b = TET + 3                                                                          # vertices 3 .. 6: vertex 3 is shared
    return np.concatenate([TET, b]).astype(np.int32), 7


def two_tets_sharing_edge():
    m = np.array([0, 1, 4, 5])                                                           # the second tetrahedron on (0, 1, 4, 5)
    return np.concatenate([TET, m[TET]]).astype(np.int32), 6


def moebius(n=8):
    """a strip of n quads closed with a half twist: 2 n vertices, 2 n faces, each quad consistently split"""
    top = lambda i: 2 * (i % n) + (1 if (i // n) % 2 else 0)
    bot = lambda i: 2 * (i % n) + (0 if (i // n) % 2 else 1)
    f = []
    for i in range(n):
        a, b, c, d = top(i), bot(i), top(i + 1), bot(i + 1)
        f += [[a, b, c], [c, b, d]]
    return np.array(f, np.int32), 2 * n


def fan(n=300):
    """n faces around the edge (0, 1), all traversing it 0 -> 1"""
    k = np.arange(n)
    return np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), k + 2], 1).astype(np.int32), n + 2


def strip(n=5000, seed=3):
    """a strip of n faces, reversed in face order, with randomly permuted vertex names"""
    i = np.arange(n, dtype=np.int64)
    f = np.stack([i, i + 1, i + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]                                                      # consistent orientation along the strip
    perm = np.random.default_rng(seed).permutation(n + 2)
    return perm[f[::-1]].astype(np.int32), n + 2


def quad_sheet(a, b, device="cuda"):
    """(faces int32 [2 a b, 3] as a torch tensor on ``device``, V): an a x b sheet of quads over (a + 1)(b + 1) vertices in row-major
    order, quad (i, j) cut into faces 2 (i b + j) and 2 (i b + j) + 1 along the same diagonal and all wound alike.  In closed form:
    E = 3 a b + a + b, 2 (a + b) boundary edges in one loop, one component, no inconsistent edge"""
    import torch
    i, j = torch.meshgrid(torch.arange(a, device=device), torch.arange(b, device=device), indexing="ij")
    v00 = (i * (b + 1) + j).reshape(-1)
    v01, v10, v11 = v00 + 1, v00 + b + 1, v00 + b + 2
    f = torch.stack([torch.stack([v00, v10, v11], 1), torch.stack([v00, v11, v01], 1)], 1)
    return f.reshape(-1, 3).to(torch.int32).contiguous(), (a + 1) * (b + 1)


def high_index_faces(V):
    """four faces of a tetrahedron on the four highest indices of V vertices"""
    return (TET + (V - 4)).astype(np.int32), V


def _mc_volume(kind, res=16, centre=(0.0, 0.0, 0.0)):
    ax = np.linspace(-1.0, 1.0, res)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    X, Y, Z = X - centre[0], Y - centre[1], Z - centre[2]
    if kind == "sphere":
        return np.sqrt(X * X + Y * Y + Z * Z) - 0.6
    return np.sqrt((np.sqrt(X * X + Y * Y) - 0.55) ** 2 + Z * Z) - 0.25


def mc_mesh(kind, res=16, centre=(0.0, 0.0, 0.0)):
    """the tests/mc_ref.py marching-cubes mesh of a sphere r = 0.6 or a torus R = 0.55, r = 0.25 on a res^3 grid over [-1, 1]^3"""
    import mc_ref
    step = 2.0 / (res - 1)
    return mc_ref.marching_cubes(_mc_volume(kind, res, centre), 0.0, (step,) * 3, (-1.0,) * 3)


def table_cases():
    """{name: (faces, n_verts, (F_c, used V, E, boundary, non-manifold, inconsistent, chi, edge components, loops))}: the hand-derived
    rows of DESIGN 4q"""
    out = {
        "tetrahedron": tetrahedron() + ((4, 4, 6, 0, 0, 0, 2, 1, 0),),
        "tetrahedron, one face reversed": tetrahedron_one_reversed() + ((4, 4, 6, 0, 0, 3, 2, 1, 0),),
        "two tetrahedra sharing a vertex": two_tets_sharing_vertex() + ((8, 7, 12, 0, 0, 0, 3, 2, 0),),
        "two tetrahedra sharing an edge": two_tets_sharing_edge() + ((8, 6, 11, 0, 1, 0, 3, 1, 0),),
        "moebius strip": moebius(8) + ((16, 16, 32, 16, 0, 1, 0, 1, 1),),
        "fan": fan(300) + ((300, 302, 601, 600, 1, 0, 1, 1, 1),),
    }
    for name, kind, centre, row in (("mc sphere", "sphere", (0.0, 0.0, 0.0), (716, 360, 1074, 0, 0, 0, 2, 1, 0)),
                                    ("mc torus", "torus", (0.0, 0.0, 0.0), (896, 448, 1344, 0, 0, 0, 0, 1, 0)),
                                    ("mc cut sphere", "sphere", (0.7, 0.0, 0.0), (518, 276, 793, 32, 0, 0, 1, 1, 1))):
        m = mc_mesh(kind, 16, centre)
        out[name] = (m["faces"], len(m["verts"]), row)
    return out


def row_of(report):
    return tuple(int(report[k]) for k in ("n_contributing", "n_used_verts", "n_edges", "n_boundary", "n_nonmanifold", "n_inconsistent",
                                          "euler", "n_components", "n_boundary_loops"))
