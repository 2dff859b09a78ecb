"""Closest point on a triangle mesh without a GPU: the numpy oracle tests/p2m_ref.py against closed forms, its rules (ties, skipped
faces, invariance under a permutation of the faces), the surface="mesh" metric arithmetic, and the argument checks of the C ABI
Section 14 entry points.  The GPU tests (tests/test_mesh_closest_gpu.py) hold the kernel to this oracle bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import p2m_ref as P


def sphere_queries(n=4096, seed=0, sigma=0.8):
    return (sigma * np.random.default_rng(seed).standard_normal((n, 3))).astype(np.float32)


def box_queries():
    """inside, outside, on faces, on edges and at corners of P.box_mesh() (all exactly representable), and random ones"""
    lo, hi = np.array([-1.0, -0.5, -0.25]), np.array([1.0, 0.5, 0.25])
    special = [[0, 0, 0], [0.5, 0.25, 0.125], [-0.75, 0.375, -0.125],                 # inside
               [2, 0, 0], [0, -3, 0], [0.5, 0.25, 1.5], [3, 2, 1], [-2, -1, -0.5], [1.5, 0.75, 0],   # outside: face, edge, corner regions
               [1, 0.25, 0.125], [0, 0.5, 0], [0.25, -0.125, -0.25],                  # on faces
               [1, 0.5, 0], [-1, 0, 0.25], [0, -0.5, -0.25],                          # on edges
               [1, 0.5, 0.25], [-1, -0.5, -0.25], [1, -0.5, 0.25]]                    # at corners
    rng = np.random.default_rng(1)
    rand = rng.uniform(-2.0, 2.0, (400, 3)) * np.array([1.0, 0.5, 0.25]) * 1.5
    inner = rng.uniform(0.0, 1.0, (200, 3)) * (hi - lo) + lo
    return np.concatenate([np.array(special, np.float64), rand, inner]).astype(np.float32)


def test_box_against_the_closed_form():
    v, f = P.box_mesh()
    q = box_queries()
    face, d2, close, totals = P.closest_brute(q, v, f)
    assert totals.tolist() == [0, 0, 0] and (face >= 0).all()
    q64 = q.astype(np.float64)
    want = P.box_distance(q64)
    # Bound: with M the largest coordinate magnitude, p = (a + s ab) + t ac carries at most 3 roundings of values <= 2 M per
    # component, r = q - p one more, d2 two per component and two sums, the square root one: below 16 ulp(M) in the distance for
    # these O(1) coordinates, and the closed form itself (three squares, two sums, one root) is within 4 ulp(M).
    M = max(np.abs(q64).max(), np.abs(v).max())
    bound = 20 * np.spacing(M)
    assert np.abs(np.sqrt(d2) - want).max() <= bound, (np.abs(np.sqrt(d2) - want).max(), bound)
    # the closest point lies on the surface: its own distance to the surface is zero up to its fp32 rounding
    assert P.box_distance(close.astype(np.float64)).max() <= np.spacing(np.float32(M))
    on = want == 0
    assert on.sum() >= 9 and (d2[on] == 0).all()


def test_sphere_within_the_sag_of_the_mesh():
    v, f, n_degenerate = P.latlong_sphere(24, 48)
    assert v.shape == (1225, 3) and f.shape == (2304, 3) and n_degenerate == 96
    cause = P.face_causes(v, f)
    assert (cause == 3).sum() == n_degenerate and set(cause.tolist()) == {0, 3}
    q = sphere_queries()
    face, d2, close, totals = P.closest_brute(q, v, f)
    assert totals.tolist() == [0, 0, n_degenerate]
    assert (cause[face] == 0).all()                                   # a skipped face is never returned
    s = P.sag(v, f)
    # the widest triangles are the halves of the equatorial quads (7.5 x 7.5 degrees): circumradius half the diagonal, 0.0926 rad,
    # and 1 - cos(0.0926) = 4.28e-3
    assert 4.2e-3 < s < 4.4e-3
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    diff = np.sqrt(d2) - np.abs(1.0 - r)
    # the polyhedron is inscribed and convex: it contains the ball of radius 1 - sag and lies in the unit ball, so radially its
    # surface is between 1 - sag and 1 and the distance is within sag of |1 - r|, either sign.  The fp32 vertices are within
    # 2^-24 of the unit sphere; 2^-22 covers that on both ends.
    print("sphere: dist - |1 - r| in [%.4e, %.4e], sag %.4e" % (diff.min(), diff.max(), s))
    assert diff.min() >= -(s + 2.0 ** -22), (diff.min(), s)
    assert diff.max() <= s + 2.0 ** -22, (diff.max(), s)


def test_permuting_the_faces_changes_nothing():
    """Queries strictly inside the convex mesh: the closest point of such a query lies in the interior of one face (the face
    whose plane is nearest), two faces tie only on the medial axis, a set of measure zero -- so the share of ties this test
    tolerates is 0, and the oracle alone is held to it."""
    v, f, _ = P.latlong_sphere(24, 48)
    q = sphere_queries(3000, 5, 0.4)
    q = q[np.linalg.norm(q, axis=1) < 0.9][:1024]
    assert q.shape[0] == 1024
    face, d2, close, totals = P.closest_brute(q, v, f)
    perm = np.random.default_rng(2).permutation(f.shape[0])           # new face j is old face perm[j]
    face_p, d2_p, close_p, totals_p = P.closest_brute(q, v, f[perm])
    assert np.array_equal(d2_p.view(np.int64), d2.view(np.int64))
    assert np.array_equal(close_p.view(np.int32), close.view(np.int32))
    assert np.array_equal(perm[face_p], face) and np.array_equal(totals_p, totals)


def test_duplicated_faces_return_the_lower_index():
    v, f = P.box_mesh()
    q = box_queries()
    face, d2, _, _ = P.closest_brute(q, v, f)
    both = np.concatenate([f, f])
    face2, d22, _, _ = P.closest_brute(q, v, both)
    assert np.array_equal(face2, face) and np.array_equal(d22.view(np.int64), d2.view(np.int64))
    rev = np.concatenate([f[::-1], f])                                # every face also earlier in the list, in reverse order
    face3, d23, _, _ = P.closest_brute(q, v, rev)
    assert (face3 < 12).all() and np.array_equal(d23.view(np.int64), d2.view(np.int64))
    # a corner is on three faces and more triangles: the exact tie goes to the lowest index
    corner = np.array([[3, 2, 1]], np.float32)
    fc, dc, pc, _ = P.closest_brute(corner, v, f)
    touching = [i for i in range(12) if 7 in f[i]]
    assert fc[0] == min(touching) and pc[0].tolist() == [1.0, 0.5, 0.25] and dc[0] == 4 + 2.25 + 0.5625


def invalid_mesh():
    """one good triangle in z = 0 and, around it, faces of every skipped kind; returns (verts, faces, totals, good face index)"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],          # 0-2 the good triangle
                  [np.nan, 0, 0], [0, np.inf, 0],           # 3, 4 non-finite
                  [2, 0, 0], [3, 0, 0],                     # 5, 6 collinear with 0, 1
                  [0, 0, 5]], np.float32)                   # 7
    f = np.array([[0, 1, -1],                               # cause 1
                  [0, 1, 8],                                # cause 1 (index V)
                  [3, 1, 9],                                # cause 1 comes before cause 2
                  [0, 1, 3],                                # cause 2 (NaN)
                  [4, 1, 2],                                # cause 2 (inf)
                  [0, 1, 2],                                # good
                  [0, 5, 6],                                # cause 3 (collinear)
                  [7, 7, 2],                                # cause 3 (repeated vertex)
                  [1, 1, 1]], np.int32)                     # cause 3
    return v, f, [3, 2, 3], 5


def test_invalid_faces_are_skipped_and_counted_by_cause():
    v, f, totals, good = invalid_mesh()
    assert P.face_causes(v, f).tolist() == [1, 1, 1, 2, 2, 0, 3, 3, 3]
    q = np.array([[0.25, 0.25, 1], [0, 0, 5], [2.5, 0, 0.1], [np.nan, 0, 0], [0, -np.inf, 0]], np.float32)
    face, d2, close, tot = P.closest_brute(q, v, f)
    assert tot.tolist() == totals
    assert face.tolist() == [good, good, good, -1, -1]
    assert d2[0] == 1.0 and close[0].tolist() == [0.25, 0.25, 0.0]
    assert d2[1] == 25.0 and d2[2] == 1.5 * 1.5 + np.float64(np.float32(0.1)) ** 2
    assert np.isnan(d2[3:]).all() and np.isnan(close[3:]).all()
    face, d2, close, tot = P.closest_brute(q, v, np.delete(f, good, 0))          # nothing usable
    assert face.tolist() == [-1] * 5 and (d2[:3] == np.inf).all() and np.isnan(d2[3:]).all() and np.isnan(close).all()
    assert tot.tolist() == totals


def test_surface_metric_arithmetic():
    from nicer_slam_amd import mesh_eval as M
    acc = np.array([0.0, 0.010, 0.0100001, 0.015, 0.020, 0.0200001, 0.05, 0.3])
    com = np.array([0.010, 0.05, 0.0499999, 0.02, 0.1, 0.0])
    dot_acc = np.array([1.0, -1.0, 0.5, -0.5, 0.0, 0.25, 1.0, -0.75])
    dot_com = np.array([-1.0, 1.0, 0.0, 0.5, -0.5, 0.2])
    got = M.surface_metrics(torch.from_numpy(acc), torch.from_numpy(com), torch.from_numpy(dot_acc), torch.from_numpy(dot_com))
    assert got.pop("surface") == "mesh"
    want = P.surface_metrics(acc, com, dot_acc, dot_com)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-15, abs=0), k
    assert got["accuracy"] == pytest.approx(acc.mean()) and got["completion"] == pytest.approx(com.mean())
    assert got["completion ratio"] == 4 / 6                          # strictly below 0.05: 0.05 itself is not
    assert got["normals"] == pytest.approx(0.5 * np.abs(dot_acc).mean() + 0.5 * np.abs(dot_com).mean())
    for key, p, r in (("f-score", 2 / 8, 2 / 6), ("f-score-15", 4 / 8, 2 / 6), ("f-score-20", 5 / 8, 3 / 6)):    # <=: the threshold counts
        assert got[key] == pytest.approx(2 * p * r / (p + r)), key
    far = torch.full((4,), 0.5, dtype=torch.float64)
    zero = M.surface_metrics(far, far, torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64))
    assert zero["f-score"] == 0.0 and zero["f-score-15"] == 0.0 and zero["f-score-20"] == 0.0 and zero["completion ratio"] == 0.0


def test_mesh_metrics_rejects_an_unknown_surface():
    from nicer_slam_amd import mesh_eval as M
    with pytest.raises(ValueError):
        M.mesh_metrics({}, {}, surface="points")


def test_section14_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib, EXPORTS
    NSA_EBADARG = 4
    for name in ("nsa_tri_workspace", "nsa_tri_build", "nsa_tri_query", "nsa_tri_query_counted"):
        assert name in EXPORTS
    assert lib.nsa_tri_workspace(0) == 0 and lib.nsa_tri_workspace(1 << 31) == 0
    for F in (1, 1000, 707336, (1 << 31) - 1):                         # the header's bound, a function of F alone
        assert 0 < lib.nsa_tri_workspace(F) <= 108 * F + (1 << 18) + 3072
    fake = ctypes.c_void_p(4096)                          # never dereferenced: every call below is rejected before a launch
    b = dict(v=fake, V=8, f=fake, F=4, ix=fake, tot=None)
    for key, val in (("v", None), ("f", None), ("ix", None), ("V", 0), ("F", 0), ("V", 1 << 31), ("F", 1 << 31)):
        a = dict(b, **{key: val})
        assert lib.nsa_tri_build(a["v"], a["V"], a["f"], a["F"], a["ix"], a["tot"], None) == NSA_EBADARG, key
    qa = dict(ix=fake, v=fake, V=8, f=fake, F=4, q=fake, M=5, fi=fake, d2=fake, p=None)
    for key, val in (("ix", None), ("v", None), ("f", None), ("V", 0), ("F", 0), ("q", None), ("fi", None), ("d2", None),
                     ("M", 1 << 31), ("F", 1 << 31)):
        a = dict(qa, **{key: val})
        assert lib.nsa_tri_query(a["ix"], a["v"], a["V"], a["f"], a["F"], a["q"], a["M"], a["fi"], a["d2"], a["p"],
                                 None) == NSA_EBADARG, key
    assert lib.nsa_tri_query(fake, fake, 8, fake, 4, None, 0, None, None, None, None) == 0          # M = 0: nothing to do
