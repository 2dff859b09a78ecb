"""The numpy statement of edge-collapse decimation (tests/decimate_ref.py, header Section 22) pinned without a GPU: hand
cases derived on paper, the topology theorems on closed and open inputs, the independence of a round's collapses (and its replay one
collapse at a time in both key orders), the target rule, the argument validation of the Python and C entry points, and the quality
of the result against vertex clustering (tests/simplify_ref.py) at DESIGN 4r's face counts."""
import copy
import ctypes

import numpy as np
import pytest

import decimate_ref as D
import p2m_ref
import simplify_ref
import smooth_ref as S
import topology_ref as T

QUAD = D.mesh_of(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), [[0, 1, 2], [0, 2, 3]])


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------

def test_tetrahedron_is_returned_unchanged():
    """every edge has 2 common neighbours = edge_count, but the union of the two rows is 4 < 5: the merged vertex would keep two
    neighbours and the tetrahedron would fold into two coincident faces"""
    out = D.decimate(D.mesh_of(simplify_ref.TET_V, simplify_ref.TET_F), target_faces=2)
    assert out["verts"].tobytes() == simplify_ref.TET_V.tobytes() and (out["faces"] == simplify_ref.TET_F).all()
    assert out["totals"] == dict(rounds=1, collapses=0, n_candidates=0, rej_lock=0, rej_error=0, rej_link=6, rej_fold=0, n_selected=0,
                                 n_faces=4, n_verts=4, status=0)
    assert (out["vertex_map"] == np.arange(4)).all() and (out["face_origin"] == np.arange(4)).all() and out["log"].shape == (0, 4)


def test_quad_of_two_triangles():
    """the diagonal (0, 2) joins two boundary vertices: 2 common neighbours + the virtual vertex = 3 != 2, the link rule; the four
    boundary edges pass it (1 common neighbour, union 4) and are held by the error limit: each end carries the planes of two
    perpendicular boundary lines"""
    st = D.State(QUAD["verts"], QUAD["faces"])
    table, ring = st.tables()
    assert table["edges"].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [2, 3]]
    code, cost, _ = D.evaluate(st, table, ring)
    assert code.tolist() == [D.CANDIDATE, D.REJ_LINK, D.CANDIDATE, D.CANDIDATE, D.CANDIDATE] and (cost[[0, 2, 3, 4]] > 0.1).all()
    out = D.decimate(QUAD, max_error=1e-6)
    assert out["totals"]["collapses"] == 0 and out["verts"].tobytes() == QUAD["verts"].tobytes() and (out["faces"] == QUAD["faces"]).all()
    # the initial quadric of vertex 1 by hand: the face z = 0 with n = (0, 0, 1) once, the lines y = 0 (m = e x n = (0, -1, 0), at
    # x_lo = 0) and x = 1 (e = (0, 1, 0), m = (1, 0, 0), d = -1), each with s = 1
    assert st.Q0[1].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0, 1.0, -1.0, 0.0, 0.0, 1.0, 3.0]


def test_flat_grid_keeps_its_corners_and_its_area():
    v, f = S.grid_mesh(9)
    out = D.decimate(D.mesh_of(v, f), max_error=1e-6)
    assert out["totals"]["n_candidates"] == 0 and len(out["faces"]) <= 8 and (out["verts"][:, 2] == 0).all()
    corners = [0, 8, 72, 80]
    assert (out["vertex_map"][corners] >= 0).all() and out["verts"][out["vertex_map"][corners]].tobytes() == v[corners].tobytes()
    assert abs(D.area(out["verts"], out["faces"]) - 64.0) < 1e-12
    interior = np.array([i * 9 + j for i in range(1, 8) for j in range(1, 8)])
    kept = np.unique(out["vertex_map"][out["vertex_map"] >= 0])
    assert len(kept) == len(out["verts"]) == 9 and len(np.unique(out["vertex_map"][interior])) <= 5


def test_two_tetrahedra_sharing_an_edge():
    f, V = T.two_tets_sharing_edge()
    v = S.index_only_mesh(f, V)
    out = D.decimate(D.mesh_of(v, f), target_faces=2, min_cos=0.0)
    st = out["state"]
    assert st.locked[:2].all() and not st.locked[2:].any() and not st.moved[:2].any()
    assert out["verts"][out["vertex_map"][:2]].tobytes() == v[:2].tobytes()


def test_a_nan_vertex_and_indices_outside_the_range():
    v, f = simplify_ref.icosphere(2)
    v, f = v.copy(), f.copy()
    f[3, 1], f[40, 0] = -1, len(v)
    v[17, 2] = np.nan
    out = D.decimate(D.mesh_of(v, f), target_faces=100)
    st = out["state"]
    ring17 = np.unique(f[(f == 17).any(1)])
    assert st.locked[ring17].all() and st.locked.sum() == len(ring17) and not st.moved[st.locked].any()
    assert 3 not in out["face_origin"] and 40 not in out["face_origin"] and len(out["faces"]) in (99, 100)
    assert np.isnan(out["verts"]).sum() == 1 and out["verts"][out["vertex_map"][17]].tobytes() == v[17].tobytes()


# ---- theorems ---------------------------------------------------------------------------------------------------------------------------

def _closed_inputs():
    yield "icosphere 2", simplify_ref.icosphere(2)
    yield "icosphere 3", simplify_ref.icosphere(3)
    yield "cube 8", simplify_ref.cube(8)
    for kind in ("sphere", "torus"):
        m = T.mc_mesh(kind, 16)
        yield "mc " + kind, (m["verts"], m["faces"])


@pytest.mark.parametrize("name,mesh", list(_closed_inputs()), ids=[n for n, _ in _closed_inputs()])
def test_closed_inputs_stay_closed_manifold_with_their_euler_characteristic(name, mesh):
    v, f = mesh
    before = T.topology(f, len(v))
    assert before["is_watertight"]
    for kw in (dict(target_faces=len(f) // 3, max_rounds=60), dict(max_error=0.02, max_rounds=30), dict(target_faces=12, max_rounds=60)):
        out = D.decimate(D.mesh_of(v, f), normals=None, **kw)
        after = T.topology(out["faces"], len(out["verts"]))
        assert after["is_watertight"] and after["n_nonmanifold"] == 0
        assert after["euler"] == before["euler"] and after["n_components"] == before["n_components"]
        assert len(out["faces"]) == len(f) - 2 * len(out["log"]) and out["totals"]["collapses"] == len(out["log"]) > 0
        assert (np.diff(out["face_origin"]) > 0).all() and (out["vertex_map"].max() == len(out["verts"]) - 1)


def test_open_and_non_orientable_inputs_keep_their_loops_and_euler_characteristic():
    f, V = T.moebius(24)
    cases = [S.grid_mesh(17, (5, 6, 4), 0.3), (S.index_only_mesh(f, V), f)]
    for v, f in cases:
        before = T.topology(f, len(v))
        for kw in (dict(target_faces=len(f) // 3, min_cos=0.0), dict(target_faces=len(f) // 2, boundary="fixed", min_cos=0.0)):
            out = D.decimate(D.mesh_of(v, f), normals=None, **kw)
            after = T.topology(out["faces"], len(out["verts"]))
            assert after["n_boundary_loops"] == before["n_boundary_loops"] and after["euler"] == before["euler"]
            assert after["n_nonmanifold"] == 0
            if before["n_boundary"] < before["n_used_verts"] or "boundary" not in kw:   # (every vertex of the strip is on its boundary)
                assert len(out["log"]) > 0


def _rounds_with_snapshots(mesh, **kw):
    """[(state before the round, the round's dict, state after it)]"""
    st = D.State(mesh["verts"], mesh["faces"], mesh.get("colors"))
    out = []
    for rnd in range(kw.pop("max_rounds", 30)):
        before = copy.deepcopy(st)
        r = D.run_round(st, rnd, **kw)
        if r["n_taken"] == 0:
            break
        out.append((before, r, copy.deepcopy(st)))
        if kw.get("target_faces") is not None and r["n_faces"] <= kw["target_faces"]:
            break
    return out


@pytest.mark.parametrize("name", ["icosphere", "grid with a hole"])
def test_collapses_of_a_round_are_independent_and_replay_in_any_order(name):
    mesh = D.mesh_of(*simplify_ref.icosphere(2), colors=True) if name == "icosphere" else D.mesh_of(*S.grid_mesh(9, (3, 3, 2), 0.5),
                                                                                                     colors=True)
    kw = dict(target_faces=len(mesh["faces"]) // 4, max_rounds=12)
    rounds = _rounds_with_snapshots(mesh, **kw)
    assert len(rounds) >= 3 and max(len(r["selected"]) for _, r, _ in rounds) >= 4
    for before, r, after in rounds:
        taken = r["edges"][r["selected"][:r["n_taken"]]]
        ring = r["ring"]
        near = [set(taken[i]) | {int(u) for e in taken[i] for u in ring["ring"][ring["ring_start"][e]:ring["ring_start"][e + 1]]}
                for i in range(len(taken))]
        for i in range(len(taken)):
            for j in range(len(taken)):
                assert i == j or not (near[i] & set(taken[j])), "an end within one edge of another collapse's end"
        rnd = int(after.log[-1][0])
        for order in (taken, taken[::-1]):
            st = copy.deepcopy(before)
            for lo, hi in order:
                D.run_round(st, rnd, only=(int(lo), int(hi)))                    # asserts that the edge is still a candidate
            assert (st.faces == after.faces).all() and (st.vmap == after.vmap).all() and (st.moved == after.moved).all()
            for a, b in ((st.X, after.X), (st.Q, after.Q), (st.C, after.C)):
                assert a.tobytes() == b.tobytes()
            assert sorted(st.log) == sorted(after.log)                           # the same cost bits, edge by edge


def test_target_faces_gives_n_or_n_minus_one():
    v, f = simplify_ref.icosphere(3)
    for n in (1279, 1000, 777, 300, 101, 20):
        out = D.decimate(D.mesh_of(v, f), target_faces=n, normals=None)
        assert len(out["faces"]) in (n, n - 1), n
    v, f = S.grid_mesh(17, (5, 6, 4), 0.3)                                       # boundary collapses remove one face: N exactly or N - 1
    for n in (400, 399, 250):
        assert len(D.decimate(D.mesh_of(v, f), target_faces=n, normals=None)["faces"]) in (n, n - 1), n
    assert D.decimate(D.mesh_of(v, f), target_faces=10 ** 6)["totals"]["rounds"] == 0


# ---- argument validation ----------------------------------------------------------------------------------------------------------------

def test_python_front_rejects_bad_arguments_without_a_gpu():
    import torch
    from nicer_slam_amd import mesh_decimate as M
    v, f = simplify_ref.icosphere(1)
    mesh = D.mesh_of(v, f)
    bad = [dict(), dict(target_faces=-1), dict(target_faces=2.5), dict(max_error=-1.0), dict(max_error=float("nan")),
           dict(target_faces=10, boundary="free"), dict(target_faces=10, boundary_weight=-1.0), dict(target_faces=10, min_cos=1.0),
           dict(target_faces=10, min_cos=-0.1), dict(target_faces=10, eps=float("inf")), dict(target_faces=10, max_rounds=-1),
           dict(target_faces=10, normals="keep"), dict(target_faces=10, fixed=np.zeros(3))]
    for kw in bad:
        with pytest.raises(ValueError):
            M.decimate(mesh, **kw)
    for broken in ({"verts": v}, {"verts": v[:, :2], "faces": f}, {"verts": v, "faces": f[:, :2]}, {"verts": v, "faces": f.astype(np.float32)},
                   {"verts": v.astype(np.int32), "faces": f}, {"verts": v, "faces": f, "colors": v[:5]}):
        with pytest.raises(ValueError):
            M.decimate(broken, target_faces=10)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a GPU"):
            M.decimate(mesh, target_faces=10)


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from nicer_slam_amd._native import lib
    EBADARG = 4
    fake = ctypes.c_void_p(256)
    big_f = (2 ** 31 - 1) // 6 + 1
    assert lib.nsa_mesh_decimate_state_bytes(0) == 0 and lib.nsa_mesh_decimate_state_bytes(2 ** 31) == 0
    assert lib.nsa_mesh_decimate_state_bytes(1000) >= 1000 * (8 * 17 + 4 + 2)
    assert lib.nsa_mesh_decimate_workspace(0, 10) == 0 and lib.nsa_mesh_decimate_workspace(10, 0) == 0
    assert lib.nsa_mesh_decimate_workspace(10, big_f) == 0 and lib.nsa_mesh_decimate_workspace(1000, 2000) > 0
    init = lambda *a: lib.nsa_mesh_decimate_init(*a)
    ok = [fake, None, 4, fake, 4, fake, fake, fake, fake, fake, fake, None, 0, 1.0, fake, fake, None]
    for i in (0, 3, 5, 6, 7, 8, 9, 10, 14, 15):                                      # every required pointer in turn
        a = list(ok)
        a[i] = None
        assert init(*a) == EBADARG, i
    for i, x in ((12, 2), (12, -1), (13, -1.0), (13, float("nan")), (13, float("inf")), (2, 2 ** 31), (4, big_f)):
        a = list(ok)
        a[i] = x
        assert init(*a) == EBADARG, (i, x)
    assert init(None, None, 0, None, 4, None, None, None, None, None, None, None, 0, 1.0, None, None, None) == 0      # V = 0: nothing to do
    assert init(None, None, 4, None, 0, None, None, None, None, None, None, None, 1, 1.0, None, None, None) == 0      # F = 0
    rnd = lambda *a: lib.nsa_mesh_decimate_round(*a)
    ok = [4, fake, 4, fake, fake, fake, fake, fake, fake, fake, fake, 0, 1, 2, 0, 0.0, 0.04, 1e-3, 0, fake, fake, fake, 4, fake, None]
    for i in (1, 3, 4, 5, 6, 7, 8, 9, 10, 19, 20, 21, 23):
        a = list(ok)
        a[i] = None
        assert rnd(*a) == EBADARG, i
    for i, x in ((16, 1.0), (16, -0.1), (16, float("nan")), (17, -1.0), (17, float("inf")), (0, 2 ** 31), (2, big_f)):
        a = list(ok)
        a[i] = x
        assert rnd(*a) == EBADARG, (i, x)
    a = list(ok)
    a[14], a[15] = 1, -1.0                                                           # a negative squared limit
    assert rnd(*a) == EBADARG
    a = list(ok)
    a[21], a[22] = None, 0                                                           # no log asked for: legal, so V = 0 returns 0
    a[0] = 0
    assert rnd(*a) == 0
    fin = lambda *a: lib.nsa_mesh_decimate_finish(*a)
    ok = [fake, None, 4, fake, fake, None, fake, None]
    for i in (0, 3, 4, 6):
        a = list(ok)
        a[i] = None
        assert fin(*a) == EBADARG, i
    assert fin(fake, fake, 4, fake, fake, None, fake, None) == EBADARG               # colours in without colours out
    assert fin(fake, None, 2 ** 31, fake, fake, None, fake, None) == EBADARG
    assert fin(None, None, 0, None, None, None, None, None) == 0


# ---- quality against vertex clustering ----------------------------------------------------------------------------------------------------

def _two_sided_mean(verts, faces, ref_verts, ref_faces, n=600):
    """the mean of the two one-sided mean distances between the surfaces, from area-weighted samples (p2m_ref.closest_brute)"""
    a = D.surface_samples(verts, faces, seed=1)[:n]
    b = D.surface_samples(ref_verts, ref_faces, seed=2)[:n]
    d_ab = np.sqrt(p2m_ref.closest_brute(a, ref_verts, ref_faces)[1])
    d_ba = np.sqrt(p2m_ref.closest_brute(b, verts, faces)[1])
    return 0.5 * (float(d_ab.mean()) + float(d_ba.mean()))


@pytest.fixture(scope="module")
def sphere5():
    return simplify_ref.icosphere(5)


@pytest.mark.parametrize("h", [0.10, 0.20, 0.37])
def test_decimation_is_closer_to_the_sphere_than_clustering(sphere5, h):
    """DESIGN 4r's rows of the 5-subdivision icosphere (3162, 834 and 264 faces): at the same face count the mean two-sided
    distance to the input surface is strictly below clustering's.  Measured from this oracle (DESIGN 4u's table), 600 samples a side:
    h 0.10: 5.2e-4 against 6.5e-4; h 0.20: 2.0e-3 against 2.9e-3; h 0.37: 6.7e-3 against 9.3e-3"""
    v, f = sphere5
    mesh = D.mesh_of(v, f)
    cl = simplify_ref.simplify(mesh, cell=h)
    cv, cf = cl["verts"].astype(np.float32), cl["faces"]
    out = D.decimate(mesh, target_faces=len(cf), normals=None)
    d_dec, d_cl = _two_sided_mean(out["verts"], out["faces"], v, f), _two_sided_mean(cv, cf, v, f)
    print(f"sphere h {h}: clustering F' {len(cf)} d {d_cl:.3e} V {simplify_ref.volume(cv, cf):.5f} | decimate F' {len(out['faces'])} "
          f"d {d_dec:.3e} V {simplify_ref.volume(out['verts'], out['faces']):.5f} rounds {out['totals']['rounds']}")
    assert len(out["faces"]) <= len(cf) and T.topology(out["faces"], len(out["verts"]))["is_watertight"]
    assert d_dec < d_cl


@pytest.mark.parametrize("h", [0.21, 0.30])
def test_decimation_is_closer_to_the_cube_than_clustering(h):
    """DESIGN 4r's rows of the welded cube at 32 quads a side (972 and 432 faces, origin (-1.01, -1.013, -1.017)): the mean distance
    of the result's surface from the cube's and the volume.  All 18 420 interior edges of the flat faces cost exactly 0, so the key's
    second word alone orders them: with the plain word lo << 32 | hi a round took 2 to 4 collapses on this lattice (256 rounds ended
    at 10 888 faces, 2000 at 1136) -- the reason why the word is mixed (header Section 22).  Measured from this oracle (DESIGN 4u's
    table): 972 faces in 60 rounds and 432 in 78, the surface within 1e-17 of the cube's and the volume 8 to the last bit, against
    2.6e-5 / 7.99937 and 5.2e-5 / 7.99878 for clustering"""
    v, f = simplify_ref.cube(32)
    mesh = D.mesh_of(v, f)
    cl = simplify_ref.simplify(mesh, cell=h, origin=(-1.01, -1.013, -1.017))
    cv, cf = cl["verts"].astype(np.float32), cl["faces"]
    out = D.decimate(mesh, target_faces=len(cf), normals=None)
    samples = lambda vv, ff: D.surface_samples(vv, ff, seed=1)[:2000]
    d_dec = float(simplify_ref.cube_surface_distance(samples(out["verts"], out["faces"])).mean())
    d_cl = float(simplify_ref.cube_surface_distance(samples(cv, cf)).mean())
    v_dec, v_cl = simplify_ref.volume(out["verts"], out["faces"]), simplify_ref.volume(cv, cf)
    print(f"cube h {h}: clustering F' {len(cf)} d {d_cl:.3e} V {v_cl:.5f} | decimate F' {len(out['faces'])} d {d_dec:.3e} V {v_dec:.5f} "
          f"rounds {out['totals']['rounds']}")
    assert len(out["faces"]) <= len(cf), (len(out["faces"]), len(cf), out["totals"]["rounds"])
    assert d_dec < d_cl and abs(v_dec - 8.0) < abs(v_cl - 8.0)
