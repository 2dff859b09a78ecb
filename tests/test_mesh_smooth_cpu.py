"""The numpy statement of mesh smoothing (tests/smooth_ref.py, header Section 21) pinned without a GPU on cases whose
answers are derived by hand, the argument checks of the six entry points (none launches anything) and the Python-side errors."""
import ctypes
import math

import numpy as np
import pytest

import smooth_ref as S
import topology_ref as T

NSA_EBADARG = 4


# ---- rings -----------------------------------------------------------------------------------------------------------------------------

def test_ring_of_a_tetrahedron_by_hand():
    """edges in (lo, hi) order: 01 02 03 12 13 23 = ids 0 .. 5; every row is the other three vertices, ascending"""
    f, V = T.tetrahedron()
    r = S.vertex_ring(f, V)
    assert r["ring_start"].tolist() == [0, 3, 6, 9, 12]
    assert r["ring"].tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    assert r["ring_edge"].tolist() == [0, 1, 2, 0, 3, 4, 1, 3, 5, 2, 4, 5]


def test_ring_of_the_fan_and_of_unused_vertices():
    f, V = T.fan(300)
    r = S.vertex_ring(f, V)
    deg = np.diff(r["ring_start"])
    assert deg[:2].tolist() == [301, 301] and (deg[2:] == 2).all() and r["ring_start"][-1] == 2 * 601
    assert r["ring"][:301].tolist() == list(range(1, 302)) and r["ring"][301:602].tolist() == [0] + list(range(2, 302))
    assert r["ring"][602:604].tolist() == [0, 1]
    f, V = T.high_index_faces(70000)
    r = S.vertex_ring(f, V)
    assert (np.diff(r["ring_start"])[:-4] == 0).all() and r["ring"].tolist() == [69997, 69998, 69999, 69996, 69998, 69999,
                                                                                   69996, 69997, 69999, 69996, 69997, 69998]
    for row in range(V - 4, V):                          # ascending within every row, the symmetric entry carries the same edge id
        s, e = r["ring_start"][row], r["ring_start"][row + 1]
        assert (np.diff(r["ring"][s:e]) > 0).all()
    e = r["table"]["edges"][r["ring_edge"]]
    own = np.repeat(np.arange(V), np.diff(r["ring_start"]))
    assert (np.sort(np.stack([own, r["ring"]], 1), 1) == e).all()


# ---- steps -----------------------------------------------------------------------------------------------------------------------------

def test_hexagon_fan_centre_goes_to_the_mean():
    """six faces around vertex 0; the rim has heights 1 .. 6, so the mean height is 3.5 and the rim's x and y cancel exactly in pairs"""
    rim = np.array([[2, 0], [1, 2], [-1, 2], [-2, 0], [-1, -2], [1, -2]], np.float32)
    v = np.concatenate([[[0.25, 0.5, 0.0]], np.concatenate([rim, np.arange(1, 7, dtype=np.float32)[:, None]], 1)]).astype(np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.int32)
    out, state = S.smooth_steps(v, f, [1.0], boundary="fixed")
    assert out[0].tolist() == [0.0, 0.0, 3.5] and (out[1:] == v[1:]).all()
    assert state.tolist() == [S.LIVE | S.MOVES | S.STEPS] + [S.LIVE | S.ON_BOUNDARY] * 6
    out, _ = S.smooth_steps(v, f, [0.5], boundary="fixed")                  # half way: every operation is exact here
    assert out[0].tolist() == [0.125, 0.25, 1.75]
    # along the rim ("curve") vertex 1 sees 2 and 6 only, not the centre: x = (1 + 1) / 2, y = (2 - 2) / 2, z = (2 + 6) / 2
    out, _ = S.smooth_steps(v, f, [1.0], boundary="curve")
    assert out[1].tolist() == [1.0, 0.0, 4.0] and out[0].tolist() == [0.0, 0.0, 3.5]
    out, _ = S.smooth_steps(v, f, [1.0], boundary="free")                   # vertex 1 sees 0, 2 and 6
    assert out[1].tolist() == [np.float32((0.25 + 1.0 + 1.0) / 3.0), np.float32((0.5 + 2.0 - 2.0) / 3.0), np.float32(8.0 / 3.0)]


def test_flat_regular_grid_is_a_fixed_point():
    """an interior vertex (i, j) has the neighbours (i +- 1, j), (i, j +- 1), (i + 1, j + 1), (i - 1, j - 1): their mean is (i, j),
    exactly, so with the rim held every step returns the input, and with the rim free the first step moves rim vertices only"""
    v, f = S.grid_mesh(9)
    for method in ("taubin", "laplacian"):
        out, _ = S.smooth_steps(v, f, S.factors_of(method, 5), boundary="fixed")
        assert out.tobytes() == v.tobytes()
    out, state = S.smooth_steps(v, f, [0.5], boundary="free")
    inner = (state & S.ON_BOUNDARY) == 0
    assert inner.sum() == 49 and (out[inner] == v[inner]).all() and (out[~inner] != v[~inner]).any()
    # along the rim a side vertex is the mean of its two rim neighbours as well: only the four corners move
    out, _ = S.smooth_steps(v, f, [0.5], boundary="curve")
    assert sorted(np.nonzero((out != v).any(1))[0].tolist()) == [0, 8, 72, 80]


def test_tetrahedron_after_one_step_by_hand():
    """vertices 0, 3 e_x, 3 e_y, 3 e_z: the mean of the other three is (1, 1, 1) for vertex 0 and (0, 1, 1) for vertex 1"""
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, 3]], np.float32)
    out, state = S.smooth_steps(v, T.TET, [0.5])
    assert out.tolist() == [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5]]
    assert (state == (S.LIVE | S.MOVES | S.STEPS)).all()
    out, _ = S.smooth_steps(v, T.TET, [0.5, -0.5])                          # from y: mean of the others of vertex 0 is (5/6, 5/6, 5/6)
    assert np.allclose(out[0], 0.5 - 0.5 * (5.0 / 6.0 - 0.5), rtol=0, atol=1e-7)
    out, _ = S.smooth_steps(v, T.TET, [0.5], fixed=[0, 1, 0, 0])
    assert out[1].tolist() == [3.0, 0.0, 0.0] and out[0].tolist() == [0.5, 0.5, 0.5]
    out, _ = S.smooth_steps(v, T.TET, [0.5], max_move=0.25)
    assert out.tolist() == [[0.25, 0.25, 0.25], [2.75, 0.25, 0.25], [0.25, 2.75, 0.25], [0.25, 0.25, 2.75]]
    out, _ = S.smooth_steps(v, T.TET, [])
    assert out.tobytes() == v.tobytes()


def test_non_finite_vertices_keep_their_bits_and_poison_nobody():
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, 3]], np.float32)
    v[3, 1] = np.float32(np.nan)
    v.view(np.uint32)[3, 2] = 0x7FC12345                                      # a NaN with a payload
    out, state = S.smooth_steps(v, T.TET, [0.5, 0.5, 0.5])
    assert out.view(np.uint32)[3].tolist() == v.view(np.uint32)[3].tolist() and state[3] == 0
    assert np.isfinite(out[:3]).all()
    one, _ = S.smooth_steps(v, T.TET, [0.5])                                 # vertex 0 sees 1 and 2 only: mean (1.5, 1.5, 0)
    assert one[0].tolist() == [0.75, 0.75, 0.0]


def test_every_moved_vertex_stays_in_the_bounding_box():
    """with 0 < f <= 1 a step is a convex combination of positions inside the box; the float64 roundings are far below half an fp32
    unit of the box's corners, which are fp32 numbers, so after the final rounding the statement holds exactly"""
    rng = np.random.default_rng(8)
    v, f, _ = S.noisy_icosphere(2, noise=0.2, seed=6)
    gv, gf = S.grid_mesh(17, (6, 6, 3), 0.5)
    for verts, faces in ((v, f), (gv, gf)):
        lo, hi = verts.min(0), verts.max(0)
        for boundary in S.BOUNDARY:
            out, _ = S.smooth_steps(verts, faces, rng.uniform(0.05, 1.0, 7).tolist(), boundary=boundary)
            assert (out >= lo).all() and (out <= hi).all()


def test_taubin_keeps_the_volume_and_laplacian_does_not():
    """DESIGN 4t's quality table: the unit icosphere(3) with 2 % radial noise"""
    v, f, clean = S.noisy_icosphere(3)
    vol = S.volume(clean, f)
    taubin, _ = S.smooth_steps(v, f, S.factors_of("taubin", 10))
    laplacian, _ = S.smooth_steps(v, f, S.factors_of("laplacian", 20))
    assert S.rms_radial_error(taubin) < 0.5 * S.rms_radial_error(v)
    assert abs(S.volume(taubin, f) / vol - 1.0) < 0.03
    assert S.volume(laplacian, f) < 0.9 * vol
    clamped, _ = S.smooth_steps(v, f, S.factors_of("taubin", 10), max_move=0.01)
    # the clamp is on the float64 position; the output's rounding adds half an fp32 unit of a coordinate below 2
    assert (np.abs(clamped.astype(np.float64) - v.astype(np.float64)) <= 0.01 + 2.0 ** -24).all()


def test_grid_with_a_hole_is_the_case_the_gpu_test_names():
    v, f = S.grid_mesh(17, (6, 6, 3), 0.5)
    t = T.edge_table(f, len(v))
    assert (t["n_boundary"], t["n_boundary_loops"], len(v) - t["n_used_verts"]) == (76, 2, 4)
    out = {b: S.smooth_steps(v, f, S.factors_of("taubin", 10), boundary=b)[0] for b in S.BOUNDARY}
    assert min(np.abs(out[a] - out[b]).max() for a, b in (("free", "fixed"), ("free", "curve"), ("fixed", "curve"))) > 0.2


# ---- normals ---------------------------------------------------------------------------------------------------------------------------

def test_vertex_normals_by_hand():
    """the right-angled corner of the tetrahedron 0, e_x, e_y, e_z wound outward: at vertex 0 three faces with normals -e_z, -e_y, -e_x
    of equal area and equal angle; at vertex 1 the slanted face (area normal (1, 1, 1), angle pi / 3) and two with angle pi / 4"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    s3 = 1.0 / math.sqrt(3.0)
    for w in ("area", "angle"):
        n = S.vertex_normals(v, T.TET, w)
        assert np.allclose(n[0], [-s3, -s3, -s3], rtol=0, atol=1e-7)
    n = S.vertex_normals(v, T.TET, "area")
    assert np.allclose(n[1], np.array([1, 0, 0]) / 1.0, rtol=0, atol=1e-7)    # (1, 1, 1) - e_z - e_y
    n = S.vertex_normals(v, T.TET, "angle")
    want = (math.pi / 3) * np.array([s3, s3, s3]) + (math.pi / 4) * np.array([0, 0, -1.0]) + (math.pi / 4) * np.array([0, -1.0, 0])
    assert np.allclose(n[1], want / np.linalg.norm(want), rtol=0, atol=1e-7)
    # no corner, a degenerate face, a non-finite vertex: zero vectors, nobody else is touched
    v2 = np.concatenate([v, [[5, 5, 5], [np.nan, 0, 0]]]).astype(np.float32)
    f2 = np.concatenate([T.TET, [[0, 1, 5], [0, 0, 1], [0, 1, 9]]]).astype(np.int32)
    for w in ("area", "angle"):
        n2 = S.vertex_normals(v2, f2, w)
        assert n2[:4].tobytes() == S.vertex_normals(v, T.TET, w).tobytes() and (n2[4:] == 0).all()


def test_recomputed_normals_agree_with_marching_cubes():
    m = T.mc_mesh("sphere", 16)
    for w in ("area", "angle"):
        n = S.vertex_normals(m["verts"], m["faces"], w)
        assert ((n * m["normals"]).sum(1) >= 0.989).all()


# ---- the entry points check their arguments before anything is launched ---------------------------------------------------------------

def test_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib
    fake = ctypes.c_void_p(4096)                                              # never dereferenced
    big = (2 ** 31 - 1) // 6 + 1
    one = (ctypes.c_double * 1)(0.5)
    assert lib.nsa_mesh_ring_workspace(10, 0) == 0 and lib.nsa_mesh_ring_workspace(10, big) == 0
    assert lib.nsa_mesh_ring_workspace(2 ** 31, 4) == 0 and lib.nsa_mesh_ring_workspace(10, 4) > 0
    assert lib.nsa_mesh_ring(None, None, 10, 0, None, None, None, None, None) == 0                       # no faces: nothing to do
    assert lib.nsa_mesh_ring(None, fake, 10, 4, fake, fake, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_mesh_ring(fake, fake, 10, 4, fake, fake, fake, None, None) == NSA_EBADARG
    assert lib.nsa_mesh_ring(fake, fake, 10, big, fake, fake, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_mesh_ring(fake, fake, 2 ** 31, 4, fake, fake, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_mesh_smooth_workspace(0, 4) == 0 and lib.nsa_mesh_smooth_workspace(10, big) == 0
    assert lib.nsa_mesh_smooth_workspace(10, 0) > 0 and lib.nsa_mesh_smooth_workspace(10, 4) > lib.nsa_mesh_smooth_workspace(10, 0)
    ok = lambda **k: lib.nsa_mesh_smooth(k.get("verts", fake), k.get("V", 10), k.get("F", 4), fake, fake, fake, k.get("count", fake), None,
                                         k.get("factors", one), k.get("n", 1), k.get("boundary", 2), k.get("max_move", math.inf), fake,
                                         k.get("out", fake), fake, None)
    assert ok(V=0) == 0                                                       # no vertices: nothing to do
    for bad in (dict(verts=None), dict(out=None), dict(count=None), dict(boundary=3), dict(boundary=-1), dict(max_move=0.0),
                dict(max_move=-1.0), dict(max_move=math.nan), dict(factors=(ctypes.c_double * 1)(1.5)),
                dict(factors=(ctypes.c_double * 1)(math.nan)), dict(factors=None), dict(F=big), dict(V=2 ** 31)):
        assert ok(**bad) == NSA_EBADARG, bad
    assert ok(V=0, factors=(ctypes.c_double * 1)(-1.5)) == NSA_EBADARG         # a bad factor is bad whatever the counts
    assert lib.nsa_mesh_vertex_normals_workspace(0, 4) == 0 and lib.nsa_mesh_vertex_normals_workspace(10, 0) == 0
    assert lib.nsa_mesh_vertex_normals_workspace(10, (2 ** 31 - 1) // 3 + 1) == 0 and lib.nsa_mesh_vertex_normals_workspace(10, 4) > 0
    assert lib.nsa_mesh_vertex_normals(None, 0, None, 0, 0, None, None, None) == 0
    assert lib.nsa_mesh_vertex_normals(None, 10, fake, 4, 0, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_mesh_vertex_normals(fake, 10, None, 4, 1, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_mesh_vertex_normals(fake, 10, fake, 4, 1, None, fake, None) == NSA_EBADARG
    assert lib.nsa_mesh_vertex_normals(fake, 10, fake, 4, 1, fake, None, None) == NSA_EBADARG
    assert lib.nsa_mesh_vertex_normals(fake, 10, fake, 4, 2, fake, fake, None) == NSA_EBADARG              # unknown weighting
    assert lib.nsa_mesh_vertex_normals(fake, 10, fake, (2 ** 31 - 1) // 3 + 1, 0, fake, fake, None) == NSA_EBADARG


def test_python_rejects_bad_arguments_before_the_gpu():
    from nicer_slam_amd import mesh_smooth as M
    v = np.zeros((4, 3), np.float32)
    mesh = dict(verts=v, faces=T.TET)
    for kw in (dict(lam=0.0), dict(lam=1.5), dict(lam=math.nan), dict(mu=-0.5), dict(mu=-0.2), dict(mu=-1.5), dict(mu=0.3),
               dict(method="hc"), dict(boundary="pinned"), dict(normals="face"), dict(iterations=-1), dict(iterations=2.5),
               dict(max_move=0.0), dict(max_move=-1.0), dict(fixed=np.zeros(3, bool))):
        with pytest.raises(ValueError):
            M.smooth(mesh, **kw)
    for bad in (dict(verts=np.zeros((4, 2), np.float32), faces=T.TET), dict(verts=v, faces=np.zeros((4, 4), np.int32)),
                dict(verts=v, faces=T.TET.astype(np.float32)), dict(verts=v.astype(np.int32), faces=T.TET), dict(verts=v)):
        with pytest.raises(ValueError):
            M.smooth(bad)
        with pytest.raises(ValueError):
            M.vertex_normals(bad)
    with pytest.raises(ValueError):
        M.vertex_normals(mesh, weighting="uniform")
    with pytest.raises(ValueError):
        M.vertex_ring(np.zeros((4, 2), np.int32), 4)
    assert M.factors_of("laplacian", 3, 0.25) == [0.25] * 3 and M.factors_of("taubin", 2) == [0.5, -0.53, 0.5, -0.53]
    assert M.factors_of("laplacian", 3, 0.5, mu=0.9) == [0.5] * 3              # laplacian ignores mu
    from nicer_slam_amd.inference import extract_mesh
    with pytest.raises(ValueError):
        extract_mesh(None, 8, smooth="taubin")
