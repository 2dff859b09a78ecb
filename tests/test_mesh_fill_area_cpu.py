"""The numpy statement of the minimum-area patches (tests/fill_area_ref.py; header Section 24), pinned on rows whose answers
can be derived by hand, on the theorems every fill must satisfy, and on a brute-force enumeration of all triangulations."""
import numpy as np
import pytest

import fill_area_ref as A
import fill_ref as R
import simplify_ref
import smooth_ref as S
import topology_ref as T


def _topology(m):
    return T.topology(m["faces"], len(m["verts"]))


def _areas(v, faces):
    X = np.asarray(v, np.float64)
    n = np.cross(X[faces[:, 1]] - X[faces[:, 0]], X[faces[:, 2]] - X[faces[:, 0]])
    return n, 0.5 * np.sqrt((n * n).sum(1))


def _edge_use(faces):
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = (e.min(1) << 32) | e.max(1)
    return dict(zip(*np.unique(key, return_counts=True)))


def check_theorems(mesh, ref):
    """what every fill of an input without pinch or blocked half-edge satisfies"""
    before, after = _topology(mesh), _topology(ref)
    filled = ref["area_totals"]["n_area_filled"] + (ref["totals"]["n_filled"] if len(ref["verts"]) > len(mesh["verts"]) else 0)
    assert after["euler"] == before["euler"] + filled and after["n_boundary_loops"] == before["n_boundary_loops"] - filled
    F = len(mesh["faces"])
    polar_faces = ref["totals"]["n_new_faces"] if len(ref["verts"]) > len(mesh["verts"]) else 0
    assert len(ref["faces"]) == F + polar_faces + ref["area_totals"]["n_area_faces"]
    assert ref["verts"][:len(mesh["verts"])].tobytes() == np.ascontiguousarray(mesh["verts"], np.float32).tobytes()
    assert ref["faces"][:F].tobytes() == np.ascontiguousarray(mesh["faces"], np.int32).tobytes()
    new = ref["faces"][F + polar_faces:]
    assert new.size == 0 or new.max() < len(mesh["verts"])                            # a minimum-area patch adds no vertex
    use0, use1 = _edge_use(mesh["faces"]), _edge_use(ref["faces"])
    assert all(c <= 2 or use0.get(k, 0) > 2 for k, c in use1.items())
    assert after["n_inconsistent"] == before["n_inconsistent"] and after["n_nonmanifold"] == before["n_nonmanifold"]
    again = A.fill_holes({k: ref[k] for k in ("verts", "faces")}, method="min_area")
    if ref["area_totals"]["n_selected"] == ref["area_totals"]["n_area_filled"] and filled == before["n_boundary_loops"]:
        assert len(again["faces"]) == len(ref["faces"])                               # a second call adds nothing


# ---- rows derived by hand -------------------------------------------------------------------------------------------------------------

def test_u_grid_row():
    mesh = A.u_grid()
    ref = A.fill_holes(mesh, method="auto")
    assert [R.CLASSES[c] for c in ref["ints"][:, 3]] == ["filled", "folded"] and ref["ints"][:, 1].tolist() == [32, 16]
    assert ref["area_ints"][:, 0].tolist() == [-1, 0] and ref["area"].tolist() == [0.0, 7.0]
    assert ref["area_totals"] == dict(n_selected=1, n_area_filled=1, n_area_too_many_edges=0, n_no_triangulation=0, n_area_faces=14,
                                      n_cells=256, max_n=16)
    W, J, mask = ref["tables"][1]
    free, _ = A.tables(np.asarray(mesh["verts"], np.float64)[mesh["faces"].reshape(-1)[ref["trace"]["order"][32:48]]], np.zeros_like(mask),
                       np.float64(1e-12))
    assert free[0, 15] == 7.0 and mask.sum() > 0                                      # with or without the chord rule
    _, area = _areas(mesh["verts"], ref["area_new_faces"])
    assert len(area) == 14 and (area == 0.5).all()
    check_theorems(mesh, ref)
    top = _topology(ref)
    assert top["is_watertight"] and top["is_oriented"] and top["euler"] == 2
    only = A.fill_holes(mesh, method="auto", max_edges=16)
    assert _topology(only)["euler"] == _topology(mesh)["euler"] + 1 and len(only["faces"]) == len(mesh["faces"]) + 14
    both = A.fill_holes(mesh, method="min_area")
    assert both["area"].tolist() == [64.0, 7.0] and len(both["verts"]) == 81 and len(both["faces"]) == len(mesh["faces"]) + 30 + 14
    check_theorems(mesh, both)


def test_smallest_loops():
    cases = A.small_cases()
    tet = A.fill_holes(cases["open tetrahedron"][0], method="min_area")
    assert tet["area_new_faces"].tolist() == [[3, 2, 0]] and tet["faces"][3].tolist() == [3, 2, 0]         # the missing face (0, 3, 2), rotated
    assert abs(tet["area"][0] - _areas(simplify_ref.TET_V, simplify_ref.TET_F[3:])[1][0]) < 1e-15 and _topology(tet)["is_oriented"]
    mesh = cases["grid without one cell"][0]
    one = A.fill_holes(mesh, method="min_area", max_edges=4)
    W, J, mask = one["tables"][1]
    assert one["ints"][1, 1] == 4 and not mask.any() and W[0, 3] == 1.0 and J[0, 3] == 1                 # the two diagonals tie: j = 1
    assert W[0, 2] == W[1, 3] == 0.5 and len(one["area_new_faces"]) == 2
    check_theorems(mesh, one)
    mesh = cases["grid of one cell"][0]
    cell = A.fill_holes(mesh, method="min_area")
    W, J, mask = cell["tables"][0]
    assert mask.sum() == 1 and np.isinf(W[np.nonzero(mask)]).all() and W[0, 3] == 1.0                    # the cell's own diagonal is forbidden
    assert J[0, 3] == (1 if mask[0, 2] else 2) and _topology(cell)["is_oriented"] and _topology(cell)["euler"] == 2
    check_theorems(mesh, cell)
    mesh = cases["grid with a hole"][0]
    hole = A.fill_holes(mesh, method="min_area", max_edges=12)
    n, area = _areas(mesh["verts"], hole["area_new_faces"])
    assert hole["area"][1] == 9.0 and len(area) == 10 and (area > 0).all() and area.sum() == 9.0         # no face of a collinear triple
    check_theorems(mesh, hole)


def test_refusals():
    cases = A.small_cases()
    mesh = cases["collinear tetrahedron"][0]
    for method in ("auto", "min_area"):
        ref = A.fill_holes(mesh, method=method)
        assert ref["area_ints"][:, 0].tolist() == [A.NO_TRIANGULATION] and np.isinf(ref["area"][0])
        assert ref["faces"].tobytes() == mesh["faces"].tobytes() and ref["area_totals"]["n_no_triangulation"] == 1
        assert ref["patches"]["plan_faces"].tolist() == [[-1, -1, -1]]
    f, V = T.strip(5000)
    mesh = A.mesh(S.index_only_mesh(f, V), f)
    ref = A.fill_holes(mesh, method="auto")
    assert ref["area_ints"][0].tolist() == [A.AREA_TOO_MANY, 5002, 0, 0, 0, 0] and ref["area_totals"]["n_cells"] == 0
    assert ref["faces"].tobytes() == mesh["faces"].tobytes() and not ref["tables"]
    mesh = cases["strip"][0]
    ref = A.fill_holes(mesh, method="auto")
    assert ref["area_ints"][:, 0].tolist() == [0] and _topology(ref)["euler"] == 2 and _topology(ref)["is_oriented"]
    check_theorems(mesh, ref)


def test_many_loops_of_four():
    mesh = A.grid65()
    ref = A.fill_holes(mesh, method="min_area", max_edges=4)
    assert ref["area_totals"]["n_area_filled"] == 256 and ref["area_totals"]["n_cells"] == 4096 and (ref["area"][ref["area_ints"][:, 0] == 0] == 1.0).all()
    assert ref["area_ints"][ref["area_ints"][:, 0] == 0, 5].tolist() == list(range(0, 512, 2))
    check_theorems(mesh, ref)


# ---- the collars ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(A.collar_cases()))
def test_collars(name):
    mesh, kw, P = A.collar_cases()[name]
    ref = A.fill_holes(mesh, method="min_area", **kw)
    n = len(mesh["verts"]) // 2
    assert ref["ints"][:, 1].tolist() == [n, n + 1] and ref["area_ints"][:, 0].tolist() == [0, -1]
    check_theorems(mesh, ref)
    if P is None:
        return
    assert R.CLASSES[ref["ints"][0, 3]] == "folded"                                   # the comb and the spiral are not star-shaped
    nrm, area = _areas(mesh["verts"], ref["area_new_faces"])
    want = abs(A.shoelace(P))
    assert abs(area.sum() - want) <= n * 2.0 ** -50 * want and abs(ref["area"][0] - want) <= n * 2.0 ** -50 * want
    # the band's faces along the hole turn the other way round the outline; the patch runs against the boundary half-edges
    assert (nrm[:, 2] * A.shoelace(P) < 0).all() and (nrm[:, :2] == 0).all()


# ---- brute force ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 4, 5, 6, 7, 8])
def test_brute_force(n):
    rng = np.random.default_rng(n)
    polys = [A.noisy_ring(n, seed=n).astype(np.float64), A.comb(max(n, 5))[:n].astype(np.float64),
             rng.integers(0, 3, (n, 3)).astype(np.float64)]                           # (small integers: ties and degenerate triangles)
    for P in polys:
        for forbid in (False, True):
            mask = np.zeros((n, n), bool)
            if forbid and n >= 5:
                mask[0, 2] = mask[1, n - 1] = True
            W, J = A.tables(P, mask, np.float64(1e-12))
            for (i, k), (v, j) in A.brute_force(P, mask, np.float64(1e-12)).items():
                assert W[i, k] == v or (np.isinf(W[i, k]) and np.isinf(v)), (i, k)
                assert J[i, k] == j, (i, k, J[i, k], j)
