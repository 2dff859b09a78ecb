"""Signed distance to a mesh without a GPU: the numpy oracle tests/sdf_ref.py (header Section 15) against closed forms and against
the two naive sign rules it replaces, the bound, the grid order and metric arithmetic of nicer_slam_amd/mesh_sdf.py, and the argument
checks of the C ABI entry points.  The GPU tests (tests/test_mesh_sdf_gpu.py) hold the kernels to this oracle."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import p2m_ref as P
import sdf_ref as S
from test_mesh_closest_cpu import invalid_mesh, sphere_queries

BOX_LO, BOX_HI = np.array([-1.0, -0.5, -0.25]), np.array([1.0, 0.5, 0.25])


def box_signed_queries(n=4000):
    return (np.random.default_rng(0).standard_normal((n, 3)) * np.array([1.5, 1.0, 0.6])).astype(np.float32)


def spike_queries(n=1500):
    return (np.random.default_rng(0).standard_normal((n, 3)) * 0.3 + np.array([0.0, 0.0, 0.6])).astype(np.float32)


def spike_apex_query():
    """0.05 above the apex along n0 + 0.15 (n1 + n3), normalised: outside, next to side 0, facing away from the 40 slivers"""
    v, f, apex, n = S.spike()
    d = n[0] + 0.15 * (n[1] + n[3])
    d /= np.linalg.norm(d)
    return (v[apex].astype(np.float64) + 0.05 * d)[None].astype(np.float32)


def margin(ref):
    """|e . N| / (|e| W) of the oracle's answers: how far the sign is from flipping (inf where e = 0 or there is no winner)"""
    with np.errstate(all="ignore"):
        m = np.abs(ref["edotn"]) / (ref["enorm"] * ref["W"])
    return np.where(np.isfinite(m), m, np.inf)


@functools.lru_cache(maxsize=None)
def box_case():
    v, f = P.box_mesh()
    q = box_signed_queries()
    return v, f, q, S.signed_brute(q, v, f)


@functools.lru_cache(maxsize=None)
def spike_case():
    v, f, apex, n = S.spike()
    q = spike_queries()
    return v, f, q, S.signed_brute(q, v, f)


def test_box_equals_the_closed_form_with_its_sign():
    v, f, q, ref = box_case()
    q64 = q.astype(np.float64)
    outside = (np.maximum(np.maximum(BOX_LO - q64, q64 - BOX_HI), 0.0) > 0).any(1)
    want = np.where(outside, 1.0, -1.0) * P.box_distance(q64)
    diff = np.abs(ref["dist"] - want).max()
    inside = (ref["sign"] < 0).mean()
    print("box: max |signed - closed form| %.3e, inside %.4f, features %s, min margin %.3f"
          % (diff, inside, np.unique(ref["feature"]).tolist(), margin(ref).min()))
    assert diff == 0.0                                               # every operand here is exact in float64: measured 0.0
    assert 0.04 < inside < 0.08                                      # measured 5.7 %
    assert np.unique(ref["feature"]).tolist() == [0, 1, 2, 3, 4, 5, 6]
    # the winner is Section 14's
    face, d2, close, _ = P.closest_brute(q, v, f)
    assert np.array_equal(ref["face"], face) and np.array_equal(ref["d2"].view(np.int64), d2.view(np.int64))
    assert np.array_equal(ref["closest"].view(np.int32), close.view(np.int32))
    assert margin(ref).min() > 0.3                                   # measured 0.34


def test_spike_apex_angle_weights_beat_the_unweighted_sum():
    v, f, apex, n = S.spike()
    assert f.shape[0] == 2 * 43 - 2 and int((f == apex).any(1).sum()) == 43
    q = spike_apex_query()
    ref = S.signed_brute(q, v, f)
    assert ref["feature"][0] in (1, 2, 4) and f[ref["face"][0]][{1: 0, 2: 1, 4: 2}[int(ref["feature"][0])]] == apex
    assert ref["sign"][0] == 1 and ref["dist"][0] == pytest.approx(0.05, rel=1e-6)
    incident = (f == apex).any(1)
    unweighted = float(P._dot(q.astype(np.float64)[0] - ref["p"][0], P.face_normals(v, f)[incident].sum(0)))
    print("spike apex: e . (unweighted sum of %d normals) = %.3f, e . N = %.4f, W = %.4f"
          % (incident.sum(), unweighted, ref["edotn"][0], ref["W"][0]))
    assert unweighted < 0                                            # measured -1.90 (-37.9 per unit |e|): "inside", wrongly
    # W is the solid-angle-like sum of the apex angles: 4 sides of apex angle 2 atan(w / sqrt(1 + w^2)) each, however side 2 is split
    w = math.tan(0.1)
    assert ref["W"][0] == pytest.approx(4 * 2 * math.atan(w / math.sqrt(1 + w * w)), rel=1e-6)


def test_spike_closest_face_normal_rule_is_wrong_near_the_edges():
    v, f, q, ref = spike_case()
    naive = S.closest_face_sign(q, v, f, ref)
    wrong = int((naive != ref["sign"]).sum())
    print("spike: closest-face rule disagrees on %d of %d, inside %.4f, min margin %.4f"
          % (wrong, q.shape[0], (ref["sign"] < 0).mean(), margin(ref).min()))
    assert wrong >= 1                                                # measured 53 of 1500
    assert 0 < (ref["sign"] < 0).sum() < 0.05 * q.shape[0]           # measured 0.9 % inside
    assert margin(ref).min() > 2.0 ** -36                            # measured 0.0139: the oracle's sign is nowhere in doubt
    # the truth, independently: the pyramid is convex, inside = below every face plane
    n = P.face_normals(v, f)
    a = v[f[:, 0]].astype(np.float64)
    inside = ((q.astype(np.float64)[:, None, :] - a[None]) * n[None]).sum(-1).max(1) < 0
    assert np.array_equal(ref["sign"] < 0, inside)
    # every face with its own three vertices: unwelded, a vertex or an edge sees one face, which is the closest-face rule again;
    # welded, the soup is the mesh
    soup_v, soup_f = v[f.reshape(-1)], np.arange(3 * f.shape[0], dtype=np.int32).reshape(-1, 3)
    welded, unwelded = S.signed_brute(q, soup_v, soup_f, weld=True), S.signed_brute(q, soup_v, soup_f, weld=False)
    assert np.array_equal(welded["sign"], ref["sign"]) and np.array_equal(welded["face"], ref["face"])
    assert int((unwelded["sign"] != ref["sign"]).sum()) >= 1


def test_latlong_sphere_welded_and_not():
    """The seam column and the pole rows repeat vertices.  Welded, the polyhedron is closed and the sign is that of |q| - 1 away from
    the sag.  Unwelded, the answers differ -- a seam edge counts one face (W = 1) where the welded mesh counts two -- but on a CONVEX
    mesh never in sign: inside, the closest point lies within a face; outside, e lies in the cone of the incident faces' normals,
    which all make acute angles with each other at so shallow a vertex, so every partial sum of them has e . N > 0.  The spike test
    above holds the case where the sign does change."""
    v, f, _ = P.latlong_sphere(24, 48)
    q = sphere_queries(1024)
    welded, unwelded = S.signed_brute(q, v, f, weld=True), S.signed_brute(q, v, f, weld=False)
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    clear = np.abs(r - 1.0) > P.sag(v, f) + 2.0 ** -22
    assert clear.sum() > 1000
    assert np.array_equal(welded["sign"][clear], np.where(r > 1.0, 1, -1)[clear])
    assert (welded["sign"] < 0).sum() > 100 and (welded["sign"] > 0).sum() > 100
    differs = (welded["W"] != unwelded["W"]) | (welded["N"] != unwelded["N"]).any(1)
    print("lat-long sphere: %d of %d answers differ unwelded (N or W)" % (differs.sum(), q.shape[0]))
    assert differs.sum() >= 1
    assert np.array_equal(welded["face"], unwelded["face"]) and np.array_equal(welded["feature"], unwelded["feature"])


def test_open_square_both_sides_and_beyond_the_rim():
    v, f = S.open_square()
    q = np.array([[0.25, 0.5, 1], [0.25, 0.5, -1], [2, 0.5, 0.5], [2, 0.5, -0.5], [2, 0.5, 0], [-1, -1, 2], [-1, -1, -2],
                  [0.5, 0.5, 0.25], [0.5, 0.5, -0.25]], np.float32)
    ref = S.signed_brute(q, v, f)
    assert ref["sign"].tolist() == [1, -1, 1, -1, 1, 1, -1, 1, -1]   # in the plane beyond the rim e . N = 0: +
    assert ref["feature"].tolist() == [0, 0, 6, 6, 6, 1, 1, 5, 5]      # (0.5, 0.5) is on the diagonal: edge ac of face 0 wins the tie
    assert ref["W"][2] == 1.0 and ref["N"][2].tolist() == [0.0, 0.0, 1.0]                # a boundary edge: one face
    assert ref["W"][7] == 2.0 and ref["N"][7].tolist() == [0.0, 0.0, 2.0]                # the diagonal: two
    assert ref["W"][5] == pytest.approx(math.pi / 2) and ref["dist"][5] == pytest.approx(math.sqrt(6))
    assert ref["dist"][1] == -1.0 and ref["dist"][4] == 1.0


def test_three_faces_on_one_edge():
    v, f = S.three_on_an_edge()
    q = np.array([[0.5, 0, -1], [0.5, 0.01, -1], [0.5, 0.5, -1]], np.float32)
    ref = S.signed_brute(q, v, f)
    assert ref["face"].tolist() == [0, 0, 0] and ref["feature"].tolist() == [3, 0, 0]
    assert ref["W"][0] == 3.0 and ref["N"][0].tolist() == [0.0, -1.0, 2.0]               # all three, in face order
    assert ref["sign"].tolist() == [-1, -1, -1]
    assert S.signed_brute(q, v, f, flip=True)["sign"].tolist() == [1, 1, 1]


def test_invalid_faces_take_no_part():
    v, f, totals, good = invalid_mesh()
    q = np.array([[-1, -1, 1], [0.25, 0.25, -1], [2, -1, 0.5], [np.nan, 0, 0], [0, -np.inf, 0]], np.float32)
    for weld in (True, False):
        ref = S.signed_brute(q, v, f, weld=weld)
        assert ref["face"].tolist() == [good, good, good, -1, -1]
        assert ref["feature"].tolist() == [1, 0, 2, -1, -1] and ref["sign"].tolist() == [1, -1, 1, 1, 1]
        # vertex a of the one usable face: its own right angle and nothing else, though eight skipped faces name vertices 0 and 1
        assert ref["W"][0] == pytest.approx(math.pi / 2) and ref["W"][2] == pytest.approx(math.pi / 4)
        assert np.isnan(ref["dist"][3:]).all() and np.isnan(ref["closest"][3:]).all()
    # an adjacency index out of range is never looked up: the face's corners contribute nothing, its interior keeps its own normal
    adj = f.copy()
    adj[good] = [0, 1, 99]
    ref = S.signed_brute(q, v, f, adj=adj)
    assert ref["W"].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0] and ref["sign"].tolist() == [1, -1, 1, 1, 1]
    none = S.signed_brute(q, v, np.delete(f, good, 0))
    assert none["face"].tolist() == [-1] * 5 and (none["dist"][:3] == np.inf).all() and (none["feature"] == -1).all()


def test_the_bound():
    v, f = P.box_mesh()
    q = np.array([[2, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 0]], np.float32)
    free = S.signed_brute(q, v, f)
    assert free["d2"][:3].tolist() == [1.0, 0.0, 0.0625] and free["sign"].tolist() == [1, 1, -1, 1]
    at = S.signed_brute(q, v, f, max_d2=1.0)                         # max_dist = 1: d2 = 1 exactly is inside
    for k in ("face", "feature", "sign"):
        assert np.array_equal(at[k], free[k]), k
    assert np.array_equal(at["d2"][:3], free["d2"][:3])
    below = S.signed_brute(q, v, f, max_d2=np.nextafter(1.0, 0.0))   # just outside
    assert below["face"].tolist() == [-1, free["face"][1], free["face"][2], -1]
    assert below["d2"][0] == np.inf and np.isnan(below["closest"][0]).all() and below["feature"][0] == -1 and below["sign"][0] == 1
    zero = S.signed_brute(q, v, f, max_d2=0.0)                       # only a point ON the surface is within 0
    assert zero["face"].tolist() == [-1, free["face"][1], -1, -1] and zero["d2"][1] == 0.0 and zero["sign"][1] == 1
    assert zero["dist"][:3].tolist() == [np.inf, 0.0, np.inf] and np.isnan(zero["dist"][3])
    inf = S.signed_brute(q, v, f, max_d2=np.inf)
    assert np.array_equal(inf["face"], free["face"]) and np.array_equal(inf["sign"], free["sign"])
    assert S.signed_brute(q, v, f, max_d2=0.0, flip=True)["dist"][0] == -np.inf


def test_grid_points_follow_get_grid_uniform():
    from nicer_slam_amd import inference, mesh_sdf
    R, bounds = 5, (-0.75, 1.25)
    want = inference.get_grid_uniform(R, bounds)["grid_points"]
    ax = mesh_sdf.grid_axis(R, bounds, "cpu")
    assert torch.equal(mesh_sdf.grid_points(ax, 0, R ** 3), want)
    assert torch.equal(mesh_sdf.grid_points(ax, 37, 91), want[37:91])           # a chunk in the middle
    # flat = (y, x, z): the second point moves in z, point R in x, point R * R in y
    assert want[1].tolist() == [-0.75, -0.75, -0.25] and want[R].tolist() == [-0.25, -0.75, -0.75]
    assert want[R * R].tolist() == [-0.75, -0.25, -0.75]


def test_field_metric_arithmetic():
    from nicer_slam_amd import mesh_sdf
    d = torch.tensor([0.01, -0.02, 0.05, 0.0500001, -0.05, math.inf, math.nan, 0.0, -0.03], dtype=torch.float64)
    f = torch.tensor([0.02, 0.01, 0.05, 9.0, -0.01, 0.0, 0.0, -0.001, -0.03], dtype=torch.float32)
    got = mesh_sdf.field_metrics(f, d, 0.05)
    use = [0, 1, 2, 4, 7, 8]                                         # |d| <= band, the band itself included; inf and NaN never
    err = np.abs(f.double().numpy()[use] - d.numpy()[use])
    assert got["points"] == 6
    assert got["mean abs error"] == pytest.approx(err.mean(), rel=1e-14)
    assert got["rms error"] == pytest.approx(math.sqrt((err * err).mean()), rel=1e-14)
    assert got["sign agreement"] == 4 / 6                            # points 1 (f > 0 > d) and 7 (f < 0 = d) disagree
    empty = mesh_sdf.field_metrics(f, d + 1.0, 0.05)
    assert empty["points"] == 0 and math.isnan(empty["mean abs error"]) and math.isnan(empty["sign agreement"])


def test_python_argument_errors():
    from nicer_slam_amd import mesh_eval, mesh_sdf
    assert mesh_eval._max_d2(None, "x") == math.inf and mesh_eval._max_d2(1.5, "x") == 2.25 and mesh_eval._max_d2(0, "x") == 0.0
    for bad in (-1.0, math.nan, -math.inf):
        with pytest.raises(ValueError):
            mesh_eval._max_d2(bad, "x")
    mesh = {"verts": np.zeros((3, 3), np.float32), "faces": np.zeros((1, 3), np.int32)}
    for kw in (dict(resolution=1), dict(resolution=8, grid_boundary=(1, 1)), dict(resolution=8, band=-0.1),
               dict(resolution=8, band=math.nan), dict(resolution=8, chunk=0)):
        with pytest.raises(ValueError):
            mesh_sdf.mesh_sdf_grid(mesh, **kw)
    for kw in (dict(n_points=0), dict(sigma=-1.0), dict(band=math.nan)):
        with pytest.raises(ValueError):
            mesh_sdf.sdf_field_metrics(lambda x: x[:, 0], mesh, **kw)
    for argv in (["m.ply"], ["m.ply", "--resolution", "8"], ["m.ply", "--out", "s.npy"], ["m.ply", "--points", "p.npy"],
                 ["m.ply", "--resolution", "8", "--out", "s.npy", "--out-dist", "d.npy"]):
        with pytest.raises(SystemExit):
            mesh_sdf.main(argv)


def test_section15_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib, EXPORTS
    NSA_EBADARG = 4
    names = ("nsa_tri_adjacency_workspace", "nsa_tri_adjacency_build", "nsa_tri_signed_query", "nsa_tri_signed_query_counted",
             "nsa_tri_query_bounded")
    for name in names:
        assert name in EXPORTS
    third = ((1 << 31) - 1) // 3
    for V, F in ((0, 1), (1, 0), (1 << 31, 1), (1, third + 1)):
        assert lib.nsa_tri_adjacency_workspace(V, F) == 0
    for V, F in ((1, 1), (3, 1), (1225, 2304), (353670, 707336), ((1 << 31) - 1, third)):          # the header's bound
        assert 0 < lib.nsa_tri_adjacency_workspace(V, F) <= 4 * V + 60 * F + (1 << 18) + 2048
    fake = ctypes.c_void_p(4096)                          # never dereferenced: every call below is rejected before a launch
    b = dict(v=fake, V=8, f=fake, a=fake, F=4, ad=fake)
    for key, val in (("v", None), ("f", None), ("a", None), ("ad", None), ("V", 0), ("F", 0), ("V", 1 << 31), ("F", third + 1)):
        x = dict(b, **{key: val})
        assert lib.nsa_tri_adjacency_build(x["v"], x["V"], x["f"], x["a"], x["F"], x["ad"], None) == NSA_EBADARG, key
    s = dict(ix=fake, ad=fake, v=fake, V=8, f=fake, a=fake, F=4, q=fake, M=5, d2=1.0, fi=fake, od=fake, ft=fake, sg=fake)

    def signed(x):
        return lib.nsa_tri_signed_query(x["ix"], x["ad"], x["v"], x["V"], x["f"], x["a"], x["F"], x["q"], x["M"], x["d2"], 0,
                                        x["fi"], x["od"], None, x["ft"], x["sg"], None)

    def counted(x):
        return lib.nsa_tri_signed_query_counted(x["ix"], x["ad"], x["v"], x["V"], x["f"], x["a"], x["F"], x["q"], x["M"], x["d2"], 1,
                                                x["fi"], x["od"], None, x["ft"], x["sg"], None, None, None, None, None)

    def bounded(x):
        return lib.nsa_tri_query_bounded(x["ix"], x["v"], x["V"], x["f"], x["F"], x["q"], x["M"], x["d2"], x["fi"], x["od"], None,
                                         None, None, None)

    common = (("ix", None), ("v", None), ("f", None), ("V", 0), ("F", 0), ("q", None), ("fi", None), ("od", None), ("M", 1 << 31),
              ("F", 1 << 31), ("d2", math.nan), ("d2", -1.0), ("d2", -math.inf))
    for key, val in common + (("ad", None), ("a", None), ("ft", None), ("sg", None), ("F", third + 1)):
        assert signed(dict(s, **{key: val})) == NSA_EBADARG, key
        assert counted(dict(s, **{key: val})) == NSA_EBADARG, key
    for key, val in common:
        assert bounded(dict(s, **{key: val})) == NSA_EBADARG, key
    empty = dict(s, M=0, q=None, fi=None, od=None, ft=None, sg=None)             # M = 0: nothing to do, whatever the bound
    for d2 in (0.0, 1.0, math.inf):
        assert signed(dict(empty, d2=d2)) == 0 and counted(dict(empty, d2=d2)) == 0 and bounded(dict(empty, d2=d2)) == 0
