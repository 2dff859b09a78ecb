"""The numpy statement of k nearest neighbours and normal estimation (tests/normals_ref.py) pinned against eval_ref.nn_brute, scipy's
cKDTree and numpy's eigh; the mutants the GPU cases must catch; and the argument checks of the two C entry points.  No GPU."""
import ctypes
import functools

import numpy as np
import pytest

import eval_ref as E
import normals_ref as N

EPS = 2.0 ** -52
C_MEASURED, W_MEASURED = 2.4573, 6.5689           # see test_jacobi_against_eigh
C_BOUND, W_BOUND = 8 * C_MEASURED, 8 * W_MEASURED


def test_k_1_is_the_nearest_neighbour_reference():
    rng = np.random.default_rng(0)
    t = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    t[7] = np.nan
    t[100:110] = t[99]
    q = np.concatenate([rng.uniform(-1.2, 1.2, (200, 3)).astype(np.float32), t[99:100], [[np.inf, 0, 0]]]).astype(np.float32)
    lat, lq = N.lattice_case()
    for targets, queries, radius in ((t, q, np.inf), (t, q, 0.1), (lat, lq, np.inf), (lat, lq, 0.5 * 3 ** 0.5)):
        dist, idx, count = N.knn_brute(queries, targets, 1, radius)
        d1, i1 = E.nn_brute(queries, targets, radius)
        assert (idx[:, 0] == i1).all() and (dist[:, 0].view(np.uint32) == d1.view(np.uint32)).all()
        assert (count == (i1 >= 0)).all()


def test_index_sets_equal_ckdtree():
    """uniform clouds have no exact ties, so the set of the k nearest does not depend on the tie rule; distances to fp32 rounding"""
    from scipy.spatial import cKDTree
    for n, k in ((1000, 8), (1000, 30), (3000, 64)):
        t = N.uniform(n, seed=n + k)
        q = N.uniform_queries(n, seed=n + k)[::3]
        dist, idx, count = N.knn_brute(q, t, k)
        d, i = cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=k)
        assert (count == k).all()
        assert (np.sort(idx, 1) == np.sort(i, 1)).all()
        assert np.allclose(dist, d, rtol=1e-6, atol=1e-9)
        assert (np.diff(dist.astype(np.float64), axis=1) >= 0).all()
    dist, idx, count = N.knn_brute(q, t, 16, 0.08)                                   # the radius form: the ball's members, nearest first
    ball = cKDTree(t.astype(np.float64)).query_ball_point(q.astype(np.float64), 0.08)
    near = [j for j, b in enumerate(ball) if len(b) <= 16]
    assert len(near) > 100
    for j in near:
        members = [b for b in ball[j] if abs(np.linalg.norm(t[b].astype(np.float64) - q[j]) - 0.08) > 1e-6]
        assert set(members) <= set(idx[j, :count[j]].tolist()) <= set(ball[j]) and (idx[j, count[j]:] == -1).all()


def test_padding_and_non_finite_rows():
    t = np.float32([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0]])
    q = np.float32([[0.1, 0, 0], [0, np.nan, 0], [10, 10, 10]])
    dist, idx, count = N.knn_brute(q, t, 5)
    assert idx.tolist() == [[0, 1, 3, -1, -1], [-1] * 5, [3, 1, 0, -1, -1]] and count.tolist() == [3, 0, 3]
    assert np.isinf(dist[0, 3:]).all() and np.isnan(dist[1]).all()
    dist, idx, count = N.knn_brute(q, t, 2, max_dist=0.8)
    assert idx.tolist() == [[0, -1], [-1, -1], [-1, -1]] and count.tolist() == [1, 0, 0]
    dist, idx, count = N.knn_brute(np.float32([[0, 0, 0]]), t, 3, max_dist=1.0)      # d2 == r2 exactly: excluded
    assert idx.tolist() == [[0, -1, -1]]


@functools.lru_cache(maxsize=None)
def _family(fi):
    rng = np.random.default_rng(100 + fi)
    points, idx, count = N.neighbourhoods(N.FAMILIES[fi], 1000, rng)
    S, ok = N.scatter(points, idx, count)
    return points, idx, count, S


@pytest.mark.parametrize("fi", range(len(N.FAMILIES)), ids=N.FAMILIES)
def test_jacobi_against_eigh(fi):
    """4000 neighbourhoods of 3 .. 64 points (thin slabs, slabs at coordinate 1000, isotropic blobs, near-lattice planes; rotated, rounded to
    fp32).  Against np.linalg.eigh of the same scatter matrices, with gap = (w1 - w0) / w2 and eps = 2^-52:
      angle between the normals * gap / eps:  measured at most 2.4573 (slab 1.97, offset 1.58, blob 1.95, lattice 2.46); asserted 8 x = 19.66
      |w - w_eigh| / (w2 eps):                measured at most 6.5689;                                                  asserted 8 x = 52.55
    (both solvers carry their own rounding).  No row needed more than 5 sweeps; the cap is 16."""
    points, idx, count, S = _family(fi)
    w, V, sweeps = N.jacobi3(S)
    A = np.zeros((len(S), 3, 3))
    for s, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        A[:, a, b] = A[:, b, a] = S[:, s]
    we, Ve = np.linalg.eigh(A)
    rel = np.abs(w - we).max(1) / we[:, 2] / EPS
    n, v = V[:, :, 0], Ve[:, :, 0]
    angle = np.arctan2(np.linalg.norm(np.cross(n, v), axis=1), np.abs((n * v).sum(1)))
    gap = (we[:, 1] - we[:, 0]) / we[:, 2]
    sel = gap >= 1e-6
    c = (angle * gap / EPS)[sel]
    print(f"{N.FAMILIES[fi]}: C {c.max():.4f} (bound {C_BOUND:.2f})  eigenvalues {rel.max():.4f} eps w2 (bound {W_BOUND:.2f})  "
          f"sweeps {sweeps.max()}  rows {sel.sum()}")
    assert sel.sum() > 900
    assert c.max() <= C_BOUND
    assert rel.max() <= W_BOUND
    assert sweeps.max() < N.MAX_SWEEPS
    assert (np.diff(w, axis=1) >= 0).all()
    assert np.abs(np.einsum("mij,mik->mjk", V, V) - np.eye(3)).max() < 1e-14


def test_jacobi_special_matrices():
    """diagonal input: no sweep, equal eigenvalues keep their columns; entries that overflow theta^2; denormal off-diagonals end by
    the |a| + |g| == |a| rule, not by underflow; NaN rows stop at the cap"""
    S = np.array([[2.0, 0, 0, 1.0, 0, 1.0], [1.0, 0, 0, 1.0, 0, 1.0], [1.0, 1e-300, 0, 1e300, 0, 1.0], [1.0, 5e-324, 5e-324, 1.0, 5e-324, 2.0],
                  [np.nan, 0, 0, 1.0, 0, 1.0], [0.0, 0, 0, 0, 0, 0]])
    w, V, sweeps = N.jacobi3(S)
    assert sweeps.tolist() == [0, 0, 1, 1, 0, 0]
    assert w[0].tolist() == [1.0, 1.0, 2.0] and V[0, :, 0].tolist() == [0, 1, 0] and V[0, :, 1].tolist() == [0, 0, 1]
    assert V[1].tolist() == np.eye(3).tolist()
    assert w[2].tolist() == [1.0, 1.0, 1e300] and w[3].tolist() == [1.0, 1.0, 2.0]
    S = np.array([[np.nan, 1.0, 0, 1.0, 0, 1.0]])
    assert N.jacobi3(S)[2].tolist() == [N.MAX_SWEEPS]


def _bits_differ(a, b):
    return (np.ascontiguousarray(a).view(np.uint8) != np.ascontiguousarray(b).view(np.uint8)).any()


def test_mutants_differ_on_the_gpu_cases():
    """each wrong implementation the device could be changes at least one bit of a case of tests/test_cloud_normals_gpu.py"""
    # a one-pass scatter loses the plane at coordinate 1000
    far = N.noisy_plane(2000, offset=1000.0)[:400]
    ref, info = N.estimate_normals(far, 30)
    bad, bad_info = N.estimate_normals(far, 30, scatter_of=N.scatter_one_pass)
    assert _bits_differ(ref, bad) and _bits_differ(info["eigenvalues"], bad_info["eigenvalues"])
    assert (info["idx"] == bad_info["idx"]).all()
    w, bad_w = info["eigenvalues"][:, 0], bad_info["eigenvalues"][:, 0]              # (in float64 it costs w0 six digits, not the plane)
    assert np.abs(bad_w - w).max() > 1e4 * EPS * w.max()
    # the neighbours summed in index order, not in the query's order
    near = N.noisy_plane(2000)[:400]
    ref, info = N.estimate_normals(near, 30)
    bad, bad_info = N.estimate_normals(near, 30, scatter_of=N.scatter_index_order)
    assert _bits_differ(info["eigenvalues"], bad_info["eigenvalues"])
    # ties at the k-th place to the higher index, on the lattice
    t, q = N.lattice_case()
    for k in (1, 2, 8, 30):
        assert _bits_differ(N.knn_brute(q[::5], t, k)[1], N.knn_brute(q[::5], t, k, tie=-1)[1])
    # a fused multiply-add in d2
    t, q = N.uniform(1000), N.uniform_queries(1000)[::4]
    a, b = N.knn_brute(q, t, 8), N.knn_brute(q, t, 8, d2_of=N.d2_fma)
    assert _bits_differ(a[0], b[0])


def test_entry_points_check_their_arguments_without_a_device():
    from nicer_slam_amd._native import lib
    NSA_EBADARG = 4
    fake = ctypes.c_void_p(4096)                                                      # never dereferenced
    inf = float("inf")
    assert lib.nsa_nn_query_k(fake, 10, fake, 5, 0, inf, fake, fake, fake, None) == NSA_EBADARG            # k = 0
    assert lib.nsa_nn_query_k(fake, 10, fake, 5, 65, inf, fake, fake, fake, None) == NSA_EBADARG           # k = 65
    assert lib.nsa_nn_query_k(fake, 10, fake, 5, 8, inf, None, fake, fake, None) == NSA_EBADARG            # NULL outputs
    assert lib.nsa_nn_query_k(fake, 10, fake, 5, 8, inf, fake, None, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_query_k(fake, 10, fake, 5, 8, inf, fake, fake, None, None) == NSA_EBADARG
    assert lib.nsa_nn_query_k(fake, 10, None, 5, 8, inf, fake, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_query_k(None, 10, fake, 5, 8, inf, fake, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_query_k(fake, 10, fake, 5, 8, 0.0, fake, fake, fake, None) == NSA_EBADARG            # max_dist not > 0
    assert lib.nsa_nn_query_k(fake, 10, None, 0, 8, inf, None, None, None, None) == 0                      # no queries
    ok = (fake, 10, fake, fake, 5, 8, fake, None, 0, fake, fake, fake, None)
    change = lambda **kw: tuple(kw.get(name, v) for name, v in zip(
        ("points", "n", "idx", "count", "m", "k", "origin", "viewpoint", "rows", "normals", "eig", "valid", "stream"), ok))
    assert lib.nsa_cloud_normals(*change(k=0)) == NSA_EBADARG
    assert lib.nsa_cloud_normals(*change(k=65)) == NSA_EBADARG
    for name in ("points", "idx", "count", "origin", "normals", "valid"):
        assert lib.nsa_cloud_normals(*change(**{name: None})) == NSA_EBADARG, name
    for rows in (2, 4, 6):
        assert lib.nsa_cloud_normals(*change(viewpoint=fake, rows=rows)) == NSA_EBADARG
    assert lib.nsa_cloud_normals(*change(rows=1)) == NSA_EBADARG                                           # rows without a viewpoint
    assert lib.nsa_cloud_normals(*change(m=0, idx=None, count=None, origin=None, normals=None, valid=None)) == 0
    assert lib.nsa_cloud_normals(*change(m=0, rows=1)) == 0


def test_python_layer_checks_its_arguments():
    from nicer_slam_amd import cloud_normals, mesh_eval, mesh_register
    assert callable(cloud_normals.estimate_normals) and callable(mesh_eval.nearest_k) and callable(mesh_eval.NNIndex.knn)
    with pytest.raises(SystemExit):
        cloud_normals.main(["in.ply"])                                                # --out is required
    import inspect
    assert inspect.signature(cloud_normals.estimate_normals).parameters["k"].default == 30
    assert mesh_register.main.__module__ == "nicer_slam_amd.mesh_register"
