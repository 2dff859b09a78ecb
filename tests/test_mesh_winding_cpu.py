"""Generalised winding numbers without a GPU: the numpy oracle tests/winding_ref.py (header Section 16) against closed forms, its
rules (orientation, flip, invalid faces, non-finite queries, det == 0), the case the feature is for -- a sphere with a hole, where
the pseudo-normal sign of Section 15 calls a half-ball outside the sphere "inside" -- the error and the cost of the tree, and the
argument checks of the C ABI entry points and of the Python layer.  The GPU tests (tests/test_mesh_winding_gpu.py) hold the kernels
to this oracle."""
import ctypes
import functools
import math

import numpy as np
import pytest

import p2m_ref as P
import sdf_ref as S
import winding_ref as W
from test_mesh_closest_cpu import invalid_mesh, sphere_queries
from test_mesh_sdf_cpu import BOX_HI, BOX_LO, box_signed_queries


def _exact(v, f, q, **kw):
    return W.exact(np.asarray(q, np.float32), W.Tree(v, f), **kw)["w"]


@functools.lru_cache(maxsize=None)
def sphere_case(holed):
    """(verts, faces, tree, queries, exact w, {beta: walk}) of the closed or the holed lat-long sphere on 4097 uniform queries"""
    v, f = W.holed_sphere() if holed else P.latlong_sphere(24, 48)[:2]
    tree = W.Tree(v, f)
    q = W.cube_queries(4097, 0, 1.5)
    return v, f, tree, q, W.exact(q, tree), {beta: W.walk(q, tree, beta) for beta in (2.0, 3.0)}


def test_open_square_closed_form_on_both_sides():
    v, f = S.open_square()
    for h in (float(np.float32(0.1)), 0.5, 2.0):                                       # the fp32 query's own height
        want = 4.0 * math.atan(1.0 / (2.0 * h * math.sqrt(4.0 * h * h + 2.0))) / (4.0 * math.pi)
        w = _exact(v, f, [[0.5, 0.5, -h], [0.5, 0.5, h]])
        assert w[0] == pytest.approx(want, abs=1e-14) and w[1] == pytest.approx(-want, abs=1e-14), (h, w, want)
    assert _exact(v, f, [[0.5, 0.5, -0.5]])[0] == pytest.approx(1.0 / 6.0, abs=1e-15)


def test_a_cube_face_from_the_centre_is_a_sixth():
    v, f = P.box_mesh((-1, -1, -1), (1, 1, 1))
    for k in range(6):
        assert _exact(v, f[2 * k:2 * k + 2], [[0, 0, 0]])[0] == pytest.approx(1.0 / 6.0, abs=1e-15)
    assert _exact(v, f, [[0, 0, 0]])[0] == pytest.approx(1.0, abs=1e-15)


def test_closed_meshes_give_one_inside_and_zero_outside():
    v, f = P.box_mesh()
    q = box_signed_queries()
    q64 = q.astype(np.float64)
    outside = (np.maximum(np.maximum(BOX_LO - q64, q64 - BOX_HI), 0.0) > 0).any(1)
    w = _exact(v, f, q)
    assert outside.sum() > 1000 and (~outside).sum() > 200
    assert np.abs(w - np.where(outside, 0.0, 1.0)).max() <= 1e-12
    v, f, _ = P.latlong_sphere(24, 48)
    q = sphere_queries(512)
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    clear = np.abs(r - 1.0) > P.sag(v, f) + 2.0 ** -22
    w = _exact(v, f, q)
    assert clear.sum() > 500 and np.abs(w - np.where(r < 1.0, 1.0, 0.0))[clear].max() <= 1e-12
    assert np.abs(_exact(v, f, q, flip=True) + w).max() == 0.0                         # flip negates, bit for bit


def test_opposite_twins_cancel_and_copies_add():
    v, f = W.opposite_twins()
    # b and c change places: det is negated exactly (B x C = -(C x B) component by component), and den keeps its bits when the
    # query lies in the plane x = y, where lB = lC and dot(A, B) = dot(A, C) term by term: Omega cancels exactly
    q = np.array([[0.25, 0.25, 1], [0.25, 0.25, -1], [-1, -1, 1], [3, 3, 0.125], [0.5, 0.5, 1e-3]], np.float32)
    assert (_exact(v, f, q) == 0.0).all()
    # anywhere else den may differ in its last bit: within the rounding of one face's term
    rng = np.random.default_rng(3)
    q = rng.uniform(-2, 2, (256, 3)).astype(np.float32)
    one = _exact(v, f[:1], q)
    assert np.abs(_exact(v, f, q)).max() <= 8 * 2.0 ** -53 and np.abs(one).max() > 0.1
    v, f = W.coincident_copies(40)
    tree = W.Tree(v, f)
    assert tree.L == 2 and tree.n_nodes == 3 and tree.end.tolist() == [40, 40, 40] and tree.face.tolist() == list(range(40))
    assert np.abs(W.exact(q, tree)["w"] - 40 * one).max() <= 40 * 40 * 2.0 ** -53   # 40 additions of values up to 40 |one| <= 20


def test_invalid_faces_and_non_finite_queries():
    v, f, totals, good = invalid_mesh()
    q = np.array([[-1, -1, 1], [0.25, 0.25, -1], [2, -1, 0.5], [0.3, 0.3, 0.01], [np.nan, 0, 0], [0, -np.inf, 0]], np.float32)
    tree = W.Tree(v, f)
    assert tree.n_usable == 1 and tree.face.tolist() == [good] and tree.L == 0 and tree.n_nodes == 1
    w = W.exact(q, tree)["w"]
    only = _exact(v, f[good:good + 1], q)
    assert np.array_equal(w.view(np.int64), only.view(np.int64)) and np.isnan(w[4:]).all() and (np.abs(w[:4]) > 1e-3).all()
    for res in (W.walk(q, tree, 2.0), W.walk(q, tree, math.inf)):
        assert np.isnan(res["w"][4:]).all() and (res["accepted"][4:] == 0).all() and (res["evaluated"][4:] == 0).all()
    none = W.Tree(v, np.delete(f, good, 0))
    assert none.n_nodes == 0 and none.n_usable == 0
    for res in (W.exact(q, none), W.walk(q, none, 2.0)):
        assert (res["w"][:4] == 0.0).all() and np.isnan(res["w"][4:]).all() and (res["evaluated"] == 0).all()


def test_a_zero_determinant_gives_no_solid_angle():
    v, f = W.opposite_twins()
    f = f[:1]
    on_vertex = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    in_plane = np.array([[0.25, 0.25, 0], [2, 3, 0], [-1, 0.5, 0], [0.5, 0.5, 0]], np.float32)      # inside, outside, outside, on edge bc
    for q in (on_vertex, in_plane):
        a, b, c = (v[f[0, k]].astype(np.float64) for k in range(3))
        assert (W.solid_angle(q.astype(np.float64), a, b, c) == 0.0).all()
        w = _exact(v, f, q)
        assert (w == 0.0).all() and not np.signbit(w).any()
    # just off the plane the face fills half the sky: Omega -> 2 pi, w -> 1/2, from either side
    w = _exact(v, f, [[0.25, 0.25, -1e-6], [0.25, 0.25, 1e-6]])
    assert w[0] == pytest.approx(0.5, abs=1e-5) and w[1] == pytest.approx(-0.5, abs=1e-5)


def test_the_sphere_with_a_hole():
    """The case the feature is for.  Above the hole -- on or outside the original sphere -- the nearest surface element is the rim
    seen from its inner side, so Section 15's pseudo-normal sign says "inside"; the winding number says outside."""
    v, f = W.holed_sphere()
    assert f.shape == (1824, 3) and (P.face_causes(v, f) == 0).sum() == 1776
    q = W.HOLE_QUERIES
    assert (np.linalg.norm(q.astype(np.float64), axis=1) >= 0.85).all()
    normal = S.signed_brute(q, v, f)["sign"]
    w = _exact(v, f, q)
    print("holed sphere: pseudo-normal sign %s, winding number %s" % (normal.tolist(), np.round(w, 4).tolist()))
    assert (normal == -1).all() and (w < 0.5).all() and 0.2 < w.min() and w.max() < 0.46
    assert w[-1] == pytest.approx(0.26, abs=0.005)                                      # (0.2, 0.1, 1.1)
    # well inside the remaining shell both rules say inside, well outside it both say outside
    both = np.array([[0, 0, -0.5], [0.3, -0.2, -0.6], [0, 0, -1.5], [1.5, 0, -0.5]], np.float32)
    assert S.signed_brute(both, v, f)["sign"].tolist() == [-1, -1, 1, 1]
    assert (_exact(v, f, both) > 0.5).tolist() == [True, True, False, False]
    # the closed sphere: the two rules agree at all of these
    cv, cf, _ = P.latlong_sphere(24, 48)
    allq = np.concatenate([q, both])
    r = np.linalg.norm(allq.astype(np.float64), axis=1)
    clear = np.abs(r - 1.0) > P.sag(cv, cf) + 2.0 ** -22
    assert clear.sum() >= 9
    assert np.array_equal((S.signed_brute(allq, cv, cf)["sign"] < 0)[clear], (_exact(cv, cf, allq) > 0.5)[clear])
    assert np.array_equal((_exact(cv, cf, allq) > 0.5)[clear], (r < 1.0)[clear])


def test_the_tree_is_a_pre_order_partition():
    for holed in (False, True):
        v, f, t, q, ex, walks = sphere_case(holed)
        assert t.L == W.level_of(t.n_usable) == (4 if holed else 5) and t.n_nodes <= W.max_nodes(f.shape[0])
        assert t.level[0] == 0 and t.begin[0] == 0 and t.end[0] == t.n_usable and t.skip[0] == t.n_nodes
        k = np.arange(t.n_nodes)
        assert (t.skip > k).all() and (t.skip[t.leaf] == k[t.leaf] + 1).all() and (t.end > t.begin).all()
        inner = ~t.leaf
        assert (t.level[k[inner] + 1] == t.level[inner] + 1).all() and (t.begin[k[inner] + 1] == t.begin[inner]).all()
        assert (np.diff(t.key) >= 0).all() and np.array_equal(np.sort(t.face), np.nonzero(P.face_causes(v, f) == 0)[0])
        same = np.diff(t.key) == 0
        assert (np.diff(t.face)[same] > 0).all()                                        # ascending face index within a leaf
        again = W.Tree(v, f)
        for name in ("N", "M", "area", "P", "r2"):
            assert np.array_equal(getattr(again, name).view(np.int64), getattr(t, name).view(np.int64)), name
        # beta = +inf: the walk is the exact sum, term for term
        sub = q[:257]
        inf = W.walk(sub, t, math.inf)
        assert np.array_equal(inf["w"].view(np.int64), ex["w"][:257].view(np.int64))
        assert (inf["accepted"] == 0).all() and (inf["evaluated"] == t.n_usable).all()


def test_approximation_error_of_the_default_beta():
    """E = max |w_tree - w_exact| over 4097 uniform queries in [-1.5, 1.5]^3.  The bound 0.05 is half the margin 0.1 at which the
    classification is tested.  Measured with this oracle: closed sphere 3.66e-2 (beta = 2) and 1.30e-2 (beta = 3), holed sphere
    3.77e-2 and 1.19e-2: the default stays Barill et al.'s beta = 2."""
    for holed in (False, True):
        v, f, t, q, ex, walks = sphere_case(holed)
        E = {beta: float(np.abs(r["w"] - ex["w"]).max()) for beta, r in walks.items()}
        print("%s sphere, L = %d, %d nodes: E(beta = 2) = %.3e, E(beta = 3) = %.3e" % ("holed" if holed else "closed", t.L, t.n_nodes,
                                                                                       E[2.0], E[3.0]))
        assert E[2.0] <= 0.05
        assert E[3.0] < E[2.0]
    from nicer_slam_amd import mesh_sdf
    import inspect
    assert inspect.signature(mesh_sdf.winding_number).parameters["beta"].default == 2.0


def test_cost_does_not_scale_with_the_faces():
    for holed in (False, True):
        v, f, t, q, ex, walks = sphere_case(holed)
        for beta, r in walks.items():
            cost = (r["accepted"] + r["evaluated"]).mean()
            print("%s sphere, beta = %g: %.1f nodes accepted and %.1f faces evaluated per query of %d usable faces"
                  % ("holed" if holed else "closed", beta, r["accepted"].mean(), r["evaluated"].mean(), t.n_usable))
            if beta == 2.0:
                assert cost < t.n_usable / 4
        far = W.walk(np.array([[300, 0, 0], [0, -300, 0], [200, 200, 200]], np.float32), t, 2.0)       # 100 cube sides away
        assert (far["accepted"] <= 8 * t.L + 1).all() and (far["evaluated"] == 0).all() and (far["accepted"] >= 1).all()
        assert np.abs(far["w"]).max() < 1e-4


def test_python_argument_errors():
    from nicer_slam_amd import mesh_sdf
    mesh = {"verts": np.zeros((3, 3), np.float32), "faces": np.zeros((1, 3), np.int32)}
    pts = np.zeros((2, 3), np.float32)
    for kw in (dict(sign="closest"), dict(sign=None), dict(sign="winding", beta=0.5), dict(sign="winding", beta=math.nan),
               dict(beta=-1.0)):
        with pytest.raises(ValueError):
            mesh_sdf.signed_distance(mesh, pts, **kw)
        with pytest.raises(ValueError):
            mesh_sdf.mesh_sdf_grid(mesh, 8, **kw)
        with pytest.raises(ValueError):
            mesh_sdf.sdf_field_metrics(lambda x: x[:, 0], mesh, **kw)
    for kw in (dict(method="closest"), dict(method="winding", beta=0.99)):
        with pytest.raises(ValueError):
            mesh_sdf.contains(mesh, pts, **kw)
    assert mesh_sdf._sign_rule("normal", 2, "x") == ("normal", 2.0) and mesh_sdf._sign_rule("winding", math.inf, "x")[1] == math.inf
    for argv in (["m.ply", "--resolution", "8", "--out", "s.npy", "--out-winding", "w.npy"],
                 ["m.ply", "--resolution", "8", "--out", "s.npy", "--sign", "closest"],
                 ["m.ply", "--resolution", "8", "--out", "s.npy", "--sign", "winding", "--beta", "0.5"]):
        with pytest.raises(SystemExit):
            mesh_sdf.main(argv)


def test_section16_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib, EXPORTS
    NSA_EBADARG = 4
    for name in ("nsa_tri_winding_workspace", "nsa_tri_winding_build", "nsa_tri_winding_query"):
        assert name in EXPORTS
    assert lib.nsa_tri_winding_workspace(0) == 0 and lib.nsa_tri_winding_workspace(1 << 31) == 0
    for F in (1, 8, 9, 12, 2304, 707336, (1 << 31) - 1):                               # the header's formula, with its roundings
        K = W.max_nodes(F)
        assert K < 3.5 * F or F < 8
        assert 0 < lib.nsa_tri_winding_workspace(F) <= 256 + 24 * F + 4 + 100 * K + (1 << 18) + 12 * 256
    fake = ctypes.c_void_p(4096)                          # never dereferenced: every call below is rejected before a launch
    b = dict(v=fake, V=8, f=fake, F=4, t=fake)
    for key, val in (("v", None), ("f", None), ("t", None), ("V", 0), ("V", 1 << 31), ("F", 1 << 31)):
        x = dict(b, **{key: val})
        assert lib.nsa_tri_winding_build(x["v"], x["V"], x["f"], x["F"], x["t"], None, None) == NSA_EBADARG, key
    assert lib.nsa_tri_winding_build(None, 8, None, 0, None, None, None) == 0            # no face: nothing to do
    s = dict(t=fake, v=fake, V=8, f=fake, F=4, q=fake, M=5, beta=2.0, w=fake)

    def query(x):
        return lib.nsa_tri_winding_query(x["t"], x["v"], x["V"], x["f"], x["F"], x["q"], x["M"], x["beta"], 0, x["w"], None, None, None)

    for key, val in (("t", None), ("v", None), ("f", None), ("q", None), ("w", None), ("V", 0), ("V", 1 << 31), ("F", 1 << 31),
                     ("M", 1 << 31), ("beta", 0.5), ("beta", math.nan), ("beta", -math.inf), ("beta", 0.0)):
        assert query(dict(s, **{key: val})) == NSA_EBADARG, key
    for beta in (1.0, 2.0, math.inf):
        assert query(dict(s, M=0, q=None, w=None, beta=beta)) == 0                      # no query: nothing to do
        assert query(dict(s, F=0, t=None, f=None, beta=beta)) == 0                      # no face: nothing to do
    assert query(dict(s, M=0, beta=0.5)) == NSA_EBADARG                                 # ... but beta is checked first
